"""CPU-side checks of the FP8 KV cache ("KV8"): the format's definition in plain torch (quant.kv8_quantize / kv8_dequantize are
quantize_mx / dequantize_mx of every 64-element row of a kv head, transposed to head-major), the rule for non-finite and all-zero
blocks, the ctypes mirrors of the two extended structs against the header compiled with the host C compiler, the new symbols,
and the refusals that need no device."""
import ctypes
import os
import subprocess

import pytest
import torch

from test_lm_loss_abi_cpu import ROOT, _struct_fields

KV8_FIELDS = ["kv8_k_codes", "kv8_k_scales", "kv8_v_codes", "kv8_v_scales"]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_kv8_quantize_is_quantize_mx_of_the_head_rows(dt):
    from tcavt_amd import quant

    g = torch.Generator().manual_seed(11)
    B, L, nkv = 3, 7, 2
    x = (torch.randn(B, L, nkv * 64, generator=g) * torch.logspace(-3, 2, L)[None, :, None]).to(dt)
    codes, sb = quant.kv8_quantize(x)
    assert codes.dtype == sb.dtype == torch.uint8 and tuple(codes.shape) == (B, nkv, L, 64) and tuple(sb.shape) == (B, nkv, L, 2)
    for b in range(B):
        for h in range(nkv):
            c, s = quant.quantize_mx(x[b, :, h * 64:(h + 1) * 64].contiguous())  # rows l of (b, h): [L, 64]
            assert torch.equal(codes[b, h], c) and torch.equal(sb[b, h], s), (b, h)
    # the transposition, spelled out: plane (b, h), row l holds columns h * 64 .. of x[b, l]
    c_tok, s_tok = quant.quantize_mx(x.reshape(B * L, nkv * 64))
    assert torch.equal(codes, c_tok.view(B, L, nkv, 64).permute(0, 2, 1, 3))
    assert torch.equal(sb, s_tok.view(B, L, nkv, 2).permute(0, 2, 1, 3))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_kv8_round_trip_is_snap_mx(dt):
    from tcavt_amd import quant

    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 9, 192, generator=g).to(dt)  # |x| < 8: every code * 2^k is a normal number of dt
    codes, sb = quant.kv8_quantize(x)
    back = quant.kv8_dequantize(codes, sb, dt)
    assert back.dtype == dt and back.shape == x.shape
    assert torch.equal(back, quant.snap_mx(x.reshape(18, 192)).view(2, 9, 192))
    b64 = quant.kv8_dequantize(codes, sb, torch.float64)
    assert b64.dtype == torch.float64 and torch.equal(b64, back.double())
    # a dequantised cache is a fixed point in VALUE (its bytes may differ: an amax that rounds to 224 * 2^k takes the next smaller k)
    assert torch.equal(quant.kv8_dequantize(*quant.kv8_quantize(back), dt), back)


def test_kv8_inf_and_zero_blocks():
    from tcavt_amd import quant

    x = torch.randn(1, 4, 128, generator=torch.Generator().manual_seed(13)).half()
    x[0, 1, 70] = float("inf")  # head 1, row 1, block 0
    x[0, 2, 32:64] = 0.0  # head 0, row 2, block 1
    x[0, 3, 0:32] = x[0, 3, 0:32] * 2.0 ** -20  # fp16 subnormals
    codes, sb = quant.kv8_quantize(x)
    assert bool((codes[0, 1, 1, :32] == 0x7F).all()) and int(sb[0, 1, 1, 0]) == 127
    assert bool((codes[0, 1, 1, 32:] != 0x7F).all())  # the row's other block is untouched by it
    assert bool((codes[0, 0, 2, 32:] == 0).all()) and int(sb[0, 0, 2, 1]) == 127  # k = 0
    amax = x[0, 3, 0:32].double().abs().max().item()
    k = int(sb[0, 0, 3, 0]) - 127
    assert amax * 2.0 ** -k <= 448 < amax * 2.0 ** -(k - 1) and k < -20
    assert torch.equal(quant.kv8_dequantize(codes, sb, torch.float64)[0, 3, 0:32], quant.dequantize_mx(
        *quant.quantize_mx(x[0, 3:4, 0:32].contiguous()), torch.float64)[0])


@pytest.mark.parametrize("cname,mirror", [("tcavt_llama_stack_args", "LlamaStackArgs"), ("tcavt_decode_args", "DecodeArgs")])
def test_mirror_matches_header_layout(tmp_path, cname, mirror):
    from tcavt_amd import capi

    cls = getattr(capi, mirror)
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_]
    assert all(n in names for n in KV8_FIELDS)
    i = names.index(KV8_FIELDS[0])
    assert names[i:i + 4] == KV8_FIELDS  # four consecutive pointers
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def test_decode_args_end_with_the_kv8_fields_and_zero_means_off():
    from tcavt_amd import capi

    assert [f[0] for f in capi.DecodeArgs._fields_][-4:] == KV8_FIELDS
    assert [f[0] for f in capi.DecodeArgs._fields_][-5] == "table_packed"
    for cls in (capi.DecodeArgs, capi.LlamaStackArgs):
        a = cls()
        assert not any(getattr(a, n) for n in KV8_FIELDS)


def test_symbols_are_exported_and_abi_version_stays():
    from tcavt_amd import capi

    assert {"tcavt_kv_store8", "tcavt_attn_decode8"} <= set(capi.EXPORTED_SYMBOLS)
    handle = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(handle, "tcavt_kv_store8") and hasattr(handle, "tcavt_attn_decode8")
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


def test_entry_points_refuse_bad_arguments_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(rc, prefix, msg):
        err = lib.tcavt_last_error()
        assert rc == 1 and err.startswith(prefix) and msg in err, (rc, err)

    refused(lib.tcavt_attn_decode8(256, 256, 256, 256, None, 256, 256, 2, 4, 1, 64, 0.125, capi.F16, 0, None), b"attn_decode8:", b"null pointer")
    refused(lib.tcavt_attn_decode8(256, 256, 256, 256, 256, 256, 256, 2, 9, 1, 64, 0.125, capi.F16, 0, None), b"attn_decode8:", b"nq / nkv <= 8")
    refused(lib.tcavt_attn_decode8(256, 256, 256, 256, 256, 256, 256, 2, 4, 1, 15329, 0.125, capi.F16, 0, None), b"attn_decode8:", b"too long")
    refused(lib.tcavt_attn_decode8(256, 264, 256, 256, 256, 256, 256, 2, 4, 1, 64, 0.125, capi.F16, 0, None), b"attn_decode8:", b"16-byte aligned")
    refused(lib.tcavt_kv_store8(256, 2, 8, 8, 4, 1, capi.F16, 256, None, 256, 256, None), b"kv_store8:", b"null pointer")
    refused(lib.tcavt_kv_store8(256, 2, 8, 7, 4, 1, capi.F16, 256, 256, 256, 256, None), b"kv_store8:", b"must be >= L")
    refused(lib.tcavt_kv_store8(256, 2, 8, 8, 4, 1, capi.F32, 256, 256, 256, 256, None), b"kv_store8:", b"dtype16")
    refused(lib.tcavt_kv_store8(256, 2, 8, 8, 4, 1, capi.F16, 256, 257, 256, 256, None), b"kv_store8:", b"aligned")


def test_step_and_stack_refuse_both_cache_types_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()
    lay = (capi.LlamaLayer * 1)()
    for n in ("w_qkv", "w_o", "w_gu", "w_d"):
        setattr(lay[0], n, 256)
    d = capi.DecodeArgs()
    d.layers = lay
    for n in ("gamma_final", "rope_cos", "rope_sin", "table", "txt_mod", "cur_tok", "pos", "h16", "part", "qkv", "att", "act", "x16",
              "logits", "bad_id_flag", "k_cache", "v_cache") + tuple(KV8_FIELDS):
        setattr(d, n, 256)
    d.n_layers, d.B, d.H, d.I, d.nq, d.nkv, d.V, d.dtype16, d.kv_lmax, d.rope_L = 1, 2, 256, 512, 4, 1, 512, capi.F16, 64, 64
    assert lib.tcavt_llama_decode_step(ctypes.byref(d), None) == 1
    assert b"exclude each other" in lib.tcavt_last_error()
    d.k_cache = d.v_cache = None
    d.kv8_v_scales = None
    assert lib.tcavt_llama_decode_step(ctypes.byref(d), None) == 1
    assert b"the four kv8 planes come together" in lib.tcavt_last_error()
    d.kv8_k_codes = d.kv8_k_scales = d.kv8_v_codes = None
    assert lib.tcavt_llama_decode_step(ctypes.byref(d), None) == 1
    assert b"null pointer" in lib.tcavt_last_error()

    s = capi.LlamaStackArgs()
    s.layers = lay
    for n in ("gamma_final", "rope_cos", "rope_sin", "h16", "part", "kv_len", "qkv", "att", "act", "out16", "k_cache", "v_cache") + tuple(KV8_FIELDS):
        setattr(s, n, 256)
    s.n_layers, s.B, s.L, s.H, s.I, s.nq, s.nkv, s.dtype16, s.kv_lmax = 1, 2, 40, 256, 512, 4, 1, capi.F16, 48
    s.npart_in = lib.tcavt_norm_npart(80, 256, 512)
    assert lib.tcavt_llama_stack_forward(ctypes.byref(s), None) == 1
    assert b"exclude each other" in lib.tcavt_last_error()
    s.k_cache = s.v_cache = None
    s.kv8_k_scales = None
    assert lib.tcavt_llama_stack_forward(ctypes.byref(s), None) == 1
    assert b"the four kv8 planes come together" in lib.tcavt_last_error()
    s.kv8_k_scales, s.kv_lmax = 256, 39
    assert lib.tcavt_llama_stack_forward(ctypes.byref(s), None) == 1
    assert b"kv_lmax >= L" in lib.tcavt_last_error()


def test_generate_batch_names_the_two_legal_cache_types():
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0))
    ids = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="'fp16' or 'fp8'.*'fp4'"):
        m.mllm.generate_batch(torch.zeros(2, 1, 8), input_ids=ids, max_new_tokens=2, kv_cache="fp4")
