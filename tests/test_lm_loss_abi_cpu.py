"""CPU-side checks of the LM-loss entry points: the ctypes mirror of tcavt_lm_loss_args matches the header (compiled with
the host C compiler), argument errors are reported before anything touches a device, and MllmTrainer refuses what it does
not support."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "tcavt.h")).read()
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.split("{")[-1].strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?[A-Za-z0-9_]+(\s+const)?\s*\**(\s*const)?", "", decl)
        names += [p.strip().lstrip("*").strip() for p in decl.split(",") if p.strip()]
    return names


def test_lm_loss_args_mirror_matches_header_layout(tmp_path):
    from tcavt_amd import capi

    cls, cname = capi.LmLossArgs, "tcavt_lm_loss_args"
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


def test_new_symbols_are_declared_exported_and_abi_version_stays():
    from tcavt_amd import capi

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tcavt.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tcavt_[a-z0-9_]+)\s*\(", text))
    new = {"tcavt_lm_loss_workspace_bytes", "tcavt_lm_loss_forward", "tcavt_lm_loss_backward"}
    assert new <= declared and new <= set(capi.EXPORTED_SYMBOLS)
    assert set(capi.EXPORTED_SYMBOLS) == declared
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


def _good_args(capi):
    a = capi.LmLossArgs()
    for n in ("h16", "table", "table_t", "labels", "loss", "count", "lse", "g_out", "workspace"):
        setattr(a, n, 256)  # (never dereferenced: every call below is refused first)
    a.B, a.L, a.V, a.H, a.Nq = 2, 40, 528, 256, 8
    a.ldh, a.ldt, a.ldg = 256, 576, 256
    a.dtype16, a.grad_dtype = capi.F16, capi.BF16
    a.workspace_bytes = capi.lib().tcavt_lm_loss_workspace_bytes(a.B * a.L, a.V, a.H)
    return a


def test_argument_errors_are_reported_without_a_device():
    from tcavt_amd import capi

    lib = capi.lib()
    both = (lib.tcavt_lm_loss_forward, lib.tcavt_lm_loss_backward)

    def refused(fn, a, msg):
        rc = fn(ctypes.byref(a) if a is not None else None, None)
        err = lib.tcavt_last_error()
        assert rc == 1 and msg in err, (rc, err)

    for fn in both:
        refused(fn, None, b"null args")
        for field in ("h16", "table", "labels", "count", "lse", "workspace"):
            a = _good_args(capi)
            setattr(a, field, None)
            refused(fn, a, b"null")
        a = _good_args(capi)
        a.V = 520
        refused(fn, a, b"multiple of 16")
        a = _good_args(capi)
        a.H = 128
        refused(fn, a, b"multiple of 256")
        a = _good_args(capi)
        a.dtype16 = capi.F32
        refused(fn, a, b"dtype16")
        a = _good_args(capi)
        a.workspace_bytes -= 1
        refused(fn, a, b"workspace too small")
        a = _good_args(capi)
        a.Nq = a.L
        refused(fn, a, b"bad B / L / Nq")
    a = _good_args(capi)
    a.loss = None
    refused(lib.tcavt_lm_loss_forward, a, b"null loss")
    a = _good_args(capi)
    a.g_out = None
    refused(lib.tcavt_lm_loss_backward, a, b"g_out")
    a = _good_args(capi)
    a.grad_dtype = capi.F32
    refused(lib.tcavt_lm_loss_backward, a, b"grad_dtype")
    a = _good_args(capi)
    a.table_t = None
    refused(lib.tcavt_lm_loss_backward, a, b"table_t")
    a = _good_args(capi)
    a.ldt = 528  # V itself: not rounded up to 64
    refused(lib.tcavt_lm_loss_backward, a, b"table_t")


def test_workspace_bytes_never_holds_a_rows_by_vocabulary_array():
    from tcavt_amd import capi

    need = capi.lib().tcavt_lm_loss_workspace_bytes(8192, 128256, 2048)
    assert 0 < need <= 640 << 20
    assert need < 8192 * 128256  # less than one byte per logit
    # growing the vocabulary beyond one chunk only adds per-tile statistics (8 bytes per row and 128 columns)
    more = capi.lib().tcavt_lm_loss_workspace_bytes(8192, 2 * 128256, 2048)
    assert more - need <= 8192 * (128256 // 128 + 2) * 8 + 4096
    assert capi.lib().tcavt_lm_loss_workspace_bytes(0, 512, 256) == 0


def test_ops_reject_cpu_tensors():
    from tcavt_amd import capi, ops

    h = torch.zeros(80, 256, dtype=torch.float16)
    with pytest.raises(capi.TcavtError, match="must live on the GPU"):
        ops.lm_loss_forward(h, torch.zeros(512, 256, dtype=torch.float16), torch.zeros(2, 32, dtype=torch.int64), 8, 2, 40,
                            loss=torch.zeros(1), count=torch.zeros(1, dtype=torch.int32), lse=torch.zeros(80),
                            workspace=torch.zeros(16, dtype=torch.uint8))


def _tiny_model(lora):
    from tcavt_amd import config, model
    from tcavt_amd.weights import make_weights

    cfg = config.tiny(use_lora=lora)
    return model.MultiModalTrajectoryModel.from_config(cfg).load_weights(make_weights(cfg, 0))


def test_mllm_trainer_refuses_a_model_without_adapters():
    from tcavt_amd import training

    with pytest.raises(ValueError, match="no LoRA adapters"):
        training.MllmTrainer(_tiny_model(False))


def test_mllm_trainer_refuses_more_than_one_rank(monkeypatch):
    import torch.distributed as dist

    from tcavt_amd import training

    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(RuntimeError, match="single process"):
        training.MllmTrainer(_tiny_model(True))


def test_lm_loss_is_opt_in_in_the_signatures():
    import inspect

    from tcavt_amd import model, training

    assert list(inspect.signature(model.LlamaMultiModal.lm_forward).parameters)[1:] == [
        "vision_embs", "context_str", "input_ids", "attention_mask", "labels"]
    assert list(inspect.signature(training.MllmTrainer.__init__).parameters)[1:8] == [
        "model", "lr", "weight_decay", "betas", "eps", "max_grad_norm", "train_mllm_front"]
    assert list(inspect.signature(training.MllmTrainer.step).parameters)[1:] == ["vision_embs", "input_ids", "attention_mask", "labels"]
