"""CPU-side checks of the MX8 entry points: the ctypes mirrors of the new and the extended structs match the header (compiled
with the host C compiler), argument errors are reported with their messages before anything touches a device, and the ABI
version stays."""
import ctypes
import os
import subprocess

import pytest

from test_lm_loss_abi_cpu import ROOT, _struct_fields


@pytest.mark.parametrize("cname,mirror", [("tcavt_gemm_mx8_args", "GemmMx8Args"), ("tcavt_llama_layer", "LlamaLayer"),
                                          ("tcavt_llama_stack_args", "LlamaStackArgs")])
def test_mirror_matches_header_layout(tmp_path, cname, mirror):
    from tcavt_amd import capi

    cls = getattr(capi, mirror)
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def test_new_fields_are_appended_and_zero_means_off():
    from tcavt_amd import capi

    assert [f[0] for f in capi.LlamaLayer._fields_][-4:] == ["w_gu8", "w_gu8_scale", "w_d8", "w_d8_scale"]
    assert [f[0] for f in capi.LlamaStackArgs._fields_][-2:] == ["mx8_codes", "mx8_scales"]
    assert [f[0] for f in capi.LlamaLayer._fields_][13] == "tape_part" and [f[0] for f in capi.LlamaStackArgs._fields_][-3] == "splitk_ws_bytes"
    lay = capi.LlamaLayer()
    assert not any(getattr(lay, n) for n in ("w_gu8", "w_gu8_scale", "w_d8", "w_d8_scale"))


def test_symbols_are_exported_and_abi_version_stays():
    from tcavt_amd import capi

    assert {"tcavt_quant_mx8", "tcavt_gemm_mx8"} <= set(capi.EXPORTED_SYMBOLS)
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


def _good(capi):
    a = capi.GemmMx8Args()
    for n in ("A8", "A_scale", "W8", "W_scale", "C"):
        setattr(a, n, 256)  # (never dereferenced: every call below is refused first)
    a.M, a.N, a.K = 300, 256, 384
    a.lda = a.ldw = 384
    a.ldsa = a.ldsw = 12
    a.ldc = 256
    a.out_dtype, a.dtype16 = capi.F32, capi.F16
    return a


def test_gemm_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(a, msg):
        rc = lib.tcavt_gemm_mx8(ctypes.byref(a) if a is not None else None, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and msg in err, (rc, err)

    refused(None, b"null args")
    a = _good(capi)
    a.K, a.lda, a.ldw = 320, 320, 320
    refused(a, b"K=320 must be a multiple of 128")
    a = _good(capi)
    a.N = 192
    refused(a, b"N=192 must be a multiple of 128")
    for epi in (capi.EPI_BIAS, capi.EPI_RELU, capi.EPI_RESIDUAL, capi.EPI_ROPE, capi.EPI_SILU_MUL, capi.EPI_ROWSCALE,
                capi.EPI_ROPE | capi.EPI_ROWSCALE, capi.EPI_NORM_OUT | capi.EPI_BIAS, capi.EPI_SILU_BWD):
        a = _good(capi)
        a.epilogue = epi
        refused(a, b"unsupported epilogue")
    a = _good(capi)
    a.W_scale = None
    refused(a, b"null")
    a = _good(capi)
    a.tile = 256
    refused(a, b"tile must be 0 (auto) or 128")
    a = _good(capi)
    a.ldsa = 8
    refused(a, b"ldsa / ldsw")
    a = _good(capi)
    a.out_dtype = capi.BF16  # dtype16 is F16
    refused(a, b"a 16-bit output is of type dtype16")
    a = _good(capi)
    a.epilogue = capi.EPI_SILU_MUL | capi.EPI_ROWSCALE  # fp32 output
    refused(a, b"SILU_MUL writes a 16-bit output")
    a = _good(capi)
    a.epilogue, a.out_dtype = capi.EPI_SILU_MUL | capi.EPI_ROWSCALE, capi.F16
    refused(a, b"ROWSCALE needs rowscale_part")
    a = _good(capi)
    a.epilogue = capi.EPI_NORM_OUT
    refused(a, b"needs norm_h16 / norm_part")
    a = _good(capi)
    a.epilogue, a.C, a.norm_h16, a.norm_part, a.residual = capi.EPI_NORM_OUT | capi.EPI_RESIDUAL, None, 256, 256, 256
    refused(a, b"residual must be NULL")
    a = _good(capi)
    a.epilogue, a.norm_h16, a.norm_part, a.norm_res16 = capi.EPI_NORM_OUT, 256, 256, 256
    refused(a, b"norm_res16 goes with the 16-bit residual stream")


def test_quant_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(msg, *args):
        rc = lib.tcavt_quant_mx8(*args, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and msg in err, (rc, err)

    refused(b"null", None, 128, capi.F16, 256, 128, 256, 4, 3, 128)
    refused(b"K=192 must be a multiple of 128", 256, 192, capi.F16, 256, 192, 256, 8, 3, 192)
    refused(b"dtype16", 256, 128, capi.F32, 256, 128, 256, 4, 3, 128)
    refused(b"ldx >= K", 256, 120, capi.F16, 256, 128, 256, 4, 3, 128)
    refused(b"alignment", 264, 128, capi.F16, 256, 128, 256, 4, 3, 128)


def _stack_args(capi, keep):
    lay = (capi.LlamaLayer * 1)()
    for n in ("w_qkv", "w_o", "w_gu", "w_d", "w_gu8", "w_gu8_scale", "w_d8", "w_d8_scale"):
        setattr(lay[0], n, 256)
    keep.append(lay)
    a = capi.LlamaStackArgs()
    a.layers = lay
    for n in ("gamma_final", "rope_cos", "rope_sin", "h16", "part", "kv_len", "qkv", "att", "act", "out16", "mx8_codes", "mx8_scales"):
        setattr(a, n, 256)
    a.n_layers, a.B, a.L, a.H, a.I, a.nq, a.nkv, a.dtype16 = 1, 2, 40, 256, 512, 4, 1, capi.F16
    a.npart_in = capi.lib().tcavt_norm_npart(80, 256, 512)
    a.rms_eps = 1e-5
    return a, lay


def test_stack_refuses_mx8_layers_it_cannot_run():
    from tcavt_amd import capi

    lib = capi.lib()
    keep = []

    def refused(a, msg):
        rc = lib.tcavt_llama_stack_forward(ctypes.byref(a), None)
        err = lib.tcavt_last_error()
        assert rc == 1 and msg in err, (rc, err)

    a, lay = _stack_args(capi, keep)
    lay[0].tape_h_mid = 256
    refused(a, b"MX8 weights cannot run with a tape")
    a, lay = _stack_args(capi, keep)
    lay[0].w_d8_scale = None
    refused(a, b"the four MX8 pointers come together")
    a, lay = _stack_args(capi, keep)
    a.mx8_scales = None
    refused(a, b"need the mx8_codes / mx8_scales workspaces")
    a, lay = _stack_args(capi, keep)
    a.I = 576
    a.npart_in = lib.tcavt_norm_npart(80, 256, 576)
    refused(a, b"I %% 128 == 0".replace(b"%%", b"%"))
    a, lay = _stack_args(capi, keep)
    a.B, a.L = 1, 24  # 24 rows: the skinny forms write H / 16 partial sums per row
    a.npart_in = lib.tcavt_norm_npart(24, 256, 512)
    refused(a, b"more than 32 rows")


def test_model_switch_refuses_what_cannot_run():
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny()
    m = model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0))
    lw = m.mllm.llama_wrapper
    assert lw.mlp_precision == "fp16"
    with pytest.raises(ValueError, match="'fp16' or 'mx8'"):
        m.set_mlp_precision("fp8")
    assert m.set_mlp_precision("mx8") is m and lw.mlp_precision == "mx8"
    m.set_mlp_precision("fp16")
    assert lw.mlp_precision == "fp16"
    lw.shape.inter += 64
    try:
        with pytest.raises(ValueError, match="multiples of 128"):
            m.set_mlp_precision("mx8")
        with pytest.raises(ValueError, match="multiples of 128"):
            lw.mlp_weights("mx8")
    finally:
        lw.shape.inter -= 64
    with pytest.raises(ValueError, match="must be 'mx8'"):
        lw.mlp_weights("fp8")
