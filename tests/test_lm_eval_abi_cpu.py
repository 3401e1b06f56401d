"""CPU-side checks of the LM eval pass and the data-parallel stage-1 trainer: the ctypes mirror of tcavt_lm_eval_args matches
the header (compiled with the host C compiler), the new symbols are declared and exported at ABI version 5, argument errors
are reported before anything touches a device, and the Python signatures are the documented ones."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from tests.test_lm_loss_abi_cpu import ROOT, _struct_fields


def test_lm_eval_args_mirror_matches_header_layout(tmp_path):
    from tcavt_amd import capi

    cls, cname = capi.LmEvalArgs, "tcavt_lm_eval_args"
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


def test_lm_loss_args_are_not_extended():
    """The eval pass has a struct of its own: tcavt_lm_loss_args keeps its fields (additive change, ABI version 5)."""
    assert _struct_fields("tcavt_lm_loss_args") == [
        "h16", "ldh", "table", "table_t", "ldt", "labels", "kv_len", "B", "L", "V", "H", "Nq", "dtype16", "grad_dtype", "reserved0",
        "loss", "count", "lse", "row_loss", "flag", "g_loss", "g_out", "ldg", "workspace", "workspace_bytes"]


def test_new_symbols_are_declared_exported_and_abi_version_stays():
    from tcavt_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tcavt_[a-z0-9_]+)\s*\(", text))
    new = {"tcavt_lm_eval_workspace_bytes", "tcavt_lm_eval"}
    assert new <= declared and new <= set(capi.EXPORTED_SYMBOLS)
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5
    assert "#define TCAVT_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "tcavt.h")).read()


def _good_args(capi):
    a = capi.LmEvalArgs()
    for n in ("h16", "table", "labels", "loss", "count", "lse", "pred", "workspace"):
        setattr(a, n, 256)  # (never dereferenced: every call below is refused first)
    a.B, a.L, a.V, a.H, a.Nq = 2, 40, 528, 256, 8
    a.ldh = 256
    a.dtype16 = capi.F16
    a.workspace_bytes = capi.lib().tcavt_lm_eval_workspace_bytes(a.B * a.L, a.V, a.H)
    return a


def test_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()

    def refused(a, msg):
        rc = lib.tcavt_lm_eval(ctypes.byref(a) if a is not None else None, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and msg in err, (rc, err)

    refused(None, b"null args")
    for field in ("h16", "table", "labels", "count", "lse", "workspace", "loss", "pred"):
        a = _good_args(capi)
        setattr(a, field, None)
        refused(a, b"null")
    for field, val, msg in (("V", 520, b"multiple of 16"), ("H", 128, b"multiple of 256"), ("dtype16", capi.F32, b"dtype16"),
                            ("Nq", 40, b"bad B / L / Nq"), ("ldh", 252, b"ldh"), ("workspace", 128, b"256-byte aligned")):
        a = _good_args(capi)
        setattr(a, field, val)
        refused(a, msg)
    a = _good_args(capi)
    a.workspace_bytes -= 1
    refused(a, b"workspace too small")


def test_workspace_holds_statistics_only():
    from tcavt_amd import capi

    lib = capi.lib()
    need = lib.tcavt_lm_eval_workspace_bytes(8192, 128256, 2048)
    assert 0 < need < lib.tcavt_lm_loss_workspace_bytes(8192, 128256, 2048) and need < 640 << 20
    assert need <= 16 * 8192 * 1002 + 64 * 8192  # at most 16 bytes per (row, tile) and the row arrays
    assert need == lib.tcavt_lm_eval_workspace_bytes(8192, 128256, 4096)  # nothing in it scales with H
    assert lib.tcavt_lm_eval_workspace_bytes(0, 512, 256) == 0


def test_ops_reject_cpu_tensors():
    from tcavt_amd import capi, ops

    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    with pytest.raises(capi.TcavtError, match="must live on the GPU"):
        ops.lm_eval(torch.zeros(80, 256, dtype=torch.float16), torch.zeros(512, 256, dtype=torch.float16),
                    torch.zeros(2, 32, dtype=torch.int64), 8, 2, 40, loss=torch.zeros(1), count=i32(1), lse=torch.zeros(80),
                    pred=i32(80), workspace=torch.zeros(16, dtype=torch.uint8))


def test_signatures():
    from tcavt_amd import evaluate, model, training

    P = inspect.Parameter
    sig = inspect.signature(model.LlamaMultiModal.lm_evaluate)
    assert list(sig.parameters)[1:] == ["vision_embs", "context_str", "input_ids", "attention_mask", "labels"]
    assert all(sig.parameters[n].default is None for n in ("input_ids", "attention_mask", "labels"))
    assert hasattr(model.LlamaWithCrossAttnPEFT, "lm_eval")
    sig = inspect.signature(evaluate.evaluate_mllm)
    assert list(sig.parameters) == ["model", "batches", "process_group"] and sig.parameters["process_group"].default is None
    sig = inspect.signature(training.MllmTrainer.__init__)
    names = list(sig.parameters)
    assert names[1:8] == ["model", "lr", "weight_decay", "betas", "eps", "max_grad_norm", "train_mllm_front"]
    assert names[8:] == ["process_group", "data_parallel", "loss_normalization"]
    assert sig.parameters["data_parallel"].default is False and sig.parameters["loss_normalization"].default == "rank"
    assert sig.parameters["process_group"].default is None and sig.parameters["data_parallel"].kind == P.POSITIONAL_OR_KEYWORD
