"""The C boundary of the top-k alternatives (tcavt_logprob_topk / _workspace_bytes) -- no GPU: the symbols are exported and bound,
the ctypes mirror of tcavt_logprob_topk_args has the header's layout (through the host C compiler), every documented refusal is
reported before a device is touched and names the argument, and the workspace size is zero without rows and monotone."""
import ctypes
import os
import subprocess

import pytest

from tcavt_amd import capi
from tests.test_logprob_abi_cpu import _struct_fields, _valid as _valid_lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "tcavt_logprob_topk"
FIELDS = ["lp", "top_ids", "top_logprobs", "workspace", "workspace_bytes", "k", "reserved0"]
LP_POINTERS = ("logits", "history", "hist_len", "step", "finished", "out_tokens", "token_logprobs", "sum_logprob", "n_scored", "workspace")


def test_symbols_are_exported_and_bound():
    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in (ENTRY, ENTRY + "_workspace_bytes"):
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.lib()
    assert lib.tcavt_logprob_topk_workspace_bytes.restype is ctypes.c_int64
    assert list(lib.tcavt_logprob_topk.argtypes) == [ctypes.POINTER(capi.LogprobTopkArgs), ctypes.c_void_p]
    assert lib.tcavt_abi_version() == capi.ABI_VERSION == 5  # no existing struct or entry changed


def test_struct_mirror_matches_header_layout(tmp_path):
    cname, cls = "tcavt_logprob_topk_args", capi.LogprobTopkArgs
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]
    assert cls._fields_[0][1] is ctypes.POINTER(capi.LogprobArgs)


def _valid(k=5, form="batch", **lp_kw):
    """Arguments that pass every check (fake, 16-byte aligned pointers: a refusal never dereferences one) -> (args, lp)."""
    lp = _valid_lp(form=form, **lp_kw)
    a = capi.LogprobTopkArgs()
    a.lp = ctypes.pointer(lp)
    a.top_ids = a.top_logprobs = a.workspace = 4096
    a.k = k
    a.workspace_bytes = capi.lib().tcavt_logprob_topk_workspace_bytes(lp.rows, k)
    return a, lp


def _refused(a, *words):
    rc = capi.lib().tcavt_logprob_topk(ctypes.byref(a) if a is not None else None, None)
    msg = capi.lib().tcavt_last_error()
    assert rc == 1, (words, rc)
    assert b"logprob_topk" in msg and all(w.encode() in msg for w in words), (words, msg)


def test_every_refusal_is_reported_without_a_device():
    _refused(None, "args", "null pointer")
    a, _ = _valid()
    a.lp = None
    _refused(a, "lp is a null pointer")
    for n in ("top_ids", "top_logprobs", "workspace"):
        a, _ = _valid()
        setattr(a, n, None)
        _refused(a, n + " is a null pointer")
    # ---- everything tcavt_logprob_begin refuses of lp
    for form in ("batch", "slots", "rows"):
        for n in LP_POINTERS:
            a, lp = _valid(form=form)
            setattr(lp, n, None)
            _refused(a, "lp: ",n + " is a null pointer")
    a, lp = _valid(form="rows")
    lp.out_row = None
    _refused(a, "lp: ","out_row is a null pointer")
    for n in ("rows", "V", "hist_cap", "out_cap"):
        for bad in (0, -1):
            a, lp = _valid()
            setattr(lp, n, bad)
            _refused(a, "lp: ",f"{n} = {bad}")
    for bad in (0, -2):
        a, lp = _valid(form="rows")
        lp.n_state = bad
        _refused(a, "lp: ",f"n_state = {bad}", "slot_of_row")
    a, lp = _valid()
    lp.workspace_bytes -= 1
    _refused(a, "lp: ","workspace_bytes")
    a, lp = _valid()
    lp.workspace = 4096 + 8
    _refused(a, "lp: ","workspace", "16-byte aligned")
    # ---- k
    for bad in (0, -1, 21, 1000):
        a, _ = _valid()
        a.k = bad
        _refused(a, f"k = {bad}")
    a, _ = _valid(k=20, V=19)
    _refused(a, "k = 20", "V = 19")
    a, _ = _valid(V=262145)
    _refused(a, "V = 262145")
    # ---- alignment of the outputs, the workspace
    for n in ("top_ids", "top_logprobs"):
        for off in (1, 2, 3):
            a, _ = _valid()
            setattr(a, n, 4096 + off)
            _refused(a, n, "4-byte aligned")
    a, _ = _valid()
    a.workspace_bytes -= 1
    _refused(a, "workspace_bytes")
    a, _ = _valid()
    a.workspace_bytes = 0
    _refused(a, "workspace_bytes")
    a, _ = _valid()
    a.workspace = 4096 + 8
    _refused(a, "workspace", "16-byte aligned")


@pytest.mark.parametrize("k,V", [(1, 1), (20, 20), (20, 262144), (5, 1003)])
def test_the_bounds_themselves_are_accepted_up_to_the_launch(k, V):
    """The checks pass at the bounds: with the output pointers valid the only refusal left is one planted behind all others."""
    a, _ = _valid(k=k, V=V)
    a.workspace = 4096 + 8  # (checked last)
    _refused(a, "workspace", "16-byte aligned")


def test_workspace_bytes_is_monotone_and_zero_without_rows():
    f = capi.lib().tcavt_logprob_topk_workspace_bytes
    assert f(0, 5) == 0 and f(-3, 5) == 0
    prev = 0
    for rows in (1, 2, 3, 5, 8, 32, 33, 256):
        now = f(rows, 5)
        assert now > prev and now % 16 == 0
        prev = now
    prev = 0
    for k in range(1, 21):
        now = f(7, k)
        assert now >= prev and now >= 7 * 16 * k * 8  # an id and a score per slice candidate
        prev = now
    assert f(7, 20) > f(7, 1)
