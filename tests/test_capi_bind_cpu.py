"""capi.bind / bind_dropout / clone_layers -- the three functions every call site fills its C argument structs with -- and the
module layout around them: model.py re-exports what callers import from it, and the backward modules no longer load it."""
import ctypes
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

REEXPORTS = ["DropoutCtx", "LanePolygonEncoder", "BlipQFormer", "LlamaWithCrossAttnPEFT", "LlamaMultiModal", "SelfAttentionBlock",
             "LTSF_NLinearEncoder", "LTSF_NLinearDecoder", "TransformerLTSF", "MultiModalTrajectoryModel", "XATTN_PAD", "LORA_V",
             "GENERATION_CUTOFF_MARKER", "cut_generated_text"]


def test_bind_writes_pointers_skips_none_and_fills_keep():
    from tcavt_amd import capi

    q, att = torch.zeros(4), torch.zeros(8, dtype=torch.float16)
    a, keep = capi.CrossAttnArgs(), []
    a.ctx = 1234  # a field given as None stays as it is
    capi.bind(a, keep, q=q, ctx=None, att=att)
    assert (a.q, a.att, a.ctx, a.fh) == (q.data_ptr(), att.data_ptr(), 1234, None)
    assert len(keep) == 2 and keep[0] is q and keep[1] is att
    b = capi.CrossAttnArgs()
    capi.bind(b, q=q)  # without a keep-list
    assert b.q == q.data_ptr()


def test_bind_dropout_masks_and_takes_field_names():
    from tcavt_amd import capi, ops

    a = capi.TStackArgs()
    capi.bind_dropout(a, None, site="first_site")
    assert (a.dropout_p, a.dropout_seed, a.first_site) == (0.0, 0, 0)
    spec = (0.1, -3, (1 << 32) + 7)  # a negative seed and a site beyond 32 bits: masked as ops._drop masks them
    capi.bind_dropout(a, spec, site="first_site")
    assert (a.dropout_p, a.dropout_seed, a.first_site) == (ctypes.c_float(0.1).value, (1 << 64) - 3, 7)
    assert ops._drop(spec) == (0.1, (1 << 64) - 3, 7) and ops._drop(None) == (0.0, 0, 0)
    s = capi.LlamaStackArgs()
    capi.bind_dropout(s, (0.25, 5, 9), p="lora_dropout_p", site="lora_first_site")
    assert (s.lora_dropout_p, s.dropout_seed, s.lora_first_site) == (0.25, 5, 9)
    x = capi.CrossAttnArgs()
    capi.bind_dropout(x, (0.5, 6, 11))  # the default names
    assert (x.dropout_p, x.dropout_seed, x.dropout_site) == (0.5, 6, 11)


def test_clone_layers_copies_every_field_and_is_independent():
    from tcavt_amd import capi

    names = [n for n, _ in capi.LlamaLayer._fields_]
    src = (capi.LlamaLayer * 3)()
    for i, lyr in enumerate(src):
        for j, n in enumerate(names):
            setattr(lyr, n, 1000 * (i + 1) + j)
    dst = capi.clone_layers(src)
    assert len(dst) == 3 and ctypes.addressof(dst) != ctypes.addressof(src)
    assert [[getattr(l, n) for n in names] for l in dst] == [[1000 * (i + 1) + j for j in range(len(names))] for i in range(3)]
    dst[1].w_qkv, src[2].w_d = 5, 6  # neither side sees the other's later writes
    assert src[1].w_qkv == 2000 and dst[2].w_d == 3000 + names.index("w_d")


def test_model_reexports_every_name_used_from_outside():
    from tcavt_amd import layout, model, parts

    for n in REEXPORTS:
        assert hasattr(model, n), n
    assert model.XATTN_PAD is layout.XATTN_PAD and model.LORA_V is layout.LORA_V and model.DropoutCtx is parts.DropoutCtx


@pytest.mark.parametrize("module", ["backward", "llm_backward"])
def test_backward_modules_do_not_load_the_model(module):
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import tcavt_amd.{module}; "
            "print('tcavt_amd.model' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout.strip() == "False"
