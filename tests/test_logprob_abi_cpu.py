"""The C boundary of the generated tokens' log-probabilities (tcavt_logprob_begin / _finish / _workspace_bytes) -- no GPU: the
symbols are exported and bound, the ctypes mirror of tcavt_logprob_args has the header's layout (through the host C compiler), every
documented refusal is reported before a device is touched and names the argument, and the workspace size is monotone."""
import ctypes
import os
import re
import subprocess

import pytest

from tcavt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tcavt_logprob_begin", "tcavt_logprob_finish")
POINTERS = ("logits", "history", "hist_len", "step", "finished", "out_tokens", "token_logprobs", "sum_logprob", "n_scored", "workspace")


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


def test_symbols_are_exported_and_bound():
    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES + ("tcavt_logprob_workspace_bytes",):
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.lib()
    assert lib.tcavt_logprob_workspace_bytes.restype is ctypes.c_int64
    for name in ENTRIES:
        assert list(getattr(lib, name).argtypes) == [ctypes.POINTER(capi.LogprobArgs), ctypes.c_void_p]
    assert lib.tcavt_abi_version() == capi.ABI_VERSION == 5  # no existing struct or entry changed


def test_struct_mirror_matches_header_layout(tmp_path):
    cname, cls = "tcavt_logprob_args", capi.LogprobArgs
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_]
    assert names == ["logits", "slot_of_row", "history", "hist_len", "step", "out_row", "finished", "out_tokens", "token_logprobs",
                     "sum_logprob", "n_scored", "workspace", "workspace_bytes", "rows", "V", "n_state", "hist_cap", "out_cap"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def _valid(rows=3, V=1000, hist_cap=40, out_cap=8, form="batch"):
    """Arguments that pass every check (fake, 16-byte aligned pointers: a refusal never dereferences one)."""
    a = capi.LogprobArgs()
    for n in POINTERS:
        setattr(a, n, 4096)
    if form in ("slots", "rows"):
        a.out_row = 4096
    if form == "rows":
        a.slot_of_row, a.n_state = 4096, 4
    a.rows, a.V, a.hist_cap, a.out_cap = rows, V, hist_cap, out_cap
    a.workspace_bytes = capi.lib().tcavt_logprob_workspace_bytes(rows, hist_cap)
    return a


def _refused(entry, a, *words):
    rc = getattr(capi.lib(), entry)(ctypes.byref(a) if a is not None else None, None)
    msg = capi.lib().tcavt_last_error()
    assert rc == 1, (entry, words, rc)
    assert entry[len("tcavt_"):].encode() in msg and all(w.encode() in msg for w in words), (entry, words, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_refusal_is_reported_without_a_device(entry):
    _refused(entry, None, "args", "null pointer")
    for form in ("batch", "slots", "rows"):
        for n in POINTERS:
            a = _valid(form=form)
            setattr(a, n, None)
            _refused(entry, a, n + " is a null pointer")
    a = _valid(form="rows")
    a.out_row = None  # the rows form writes at out_row[s]
    _refused(entry, a, "out_row is a null pointer")
    for n in ("rows", "V", "hist_cap", "out_cap"):
        for bad in (0, -1):
            a = _valid()
            setattr(a, n, bad)
            _refused(entry, a, f"{n} = {bad}")
    for bad in (0, -2):
        a = _valid(form="rows")
        a.n_state = bad
        _refused(entry, a, f"n_state = {bad}", "slot_of_row")
    a = _valid()
    a.workspace_bytes -= 1
    _refused(entry, a, "workspace_bytes")
    a = _valid()
    a.workspace_bytes = 0
    _refused(entry, a, "workspace_bytes")
    a = _valid()
    a.workspace = 4096 + 8
    _refused(entry, a, "workspace", "16-byte aligned")


def test_workspace_bytes_is_monotone_and_zero_without_rows():
    f = capi.lib().tcavt_logprob_workspace_bytes
    assert f(0, 40) == 0 and f(-3, 40) == 0
    prev = 0
    for rows in (1, 2, 3, 5, 8, 32, 33, 256):
        now = f(rows, 40)
        assert now > prev and now % 16 == 0
        prev = now
    prev = 0
    for cap in (1, 2, 7, 40, 41, 300, 4096):
        now = f(5, cap)
        assert now >= prev and now >= 5 * cap * 4  # room for the raw logits at every history id
        prev = now
    assert f(5, 4096) > f(5, 40)
