"""The C boundary of constrained decoding (tcavt_constraint_build / _mask / _advance / _workspace_bytes) -- no GPU: the symbols
are exported and bound, the ctypes mirrors of tcavt_constraint_table and tcavt_constraint_args have the header's layout (through
the host C compiler), and every documented refusal is reported before a device is touched and names the argument."""
import ctypes
import os
import re
import subprocess

import pytest

from tcavt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tcavt_constraint_mask", "tcavt_constraint_advance")
TABLE_POINTERS = ("token_class", "trans", "bitmap", "count")
POINTERS = ("logits", "step", "finished", "cur_tok", "state", "start", "workspace")
STRUCTS = {
    "tcavt_constraint_table": (capi.ConstraintTable, ["token_class", "trans", "bitmap", "count", "V", "n_states", "n_classes", "reserved0"]),
    "tcavt_constraint_args": (capi.ConstraintArgs, ["table", "logits", "slot_of_row", "step", "out_row", "finished", "cur_tok", "state", "start",
                                                    "request_state", "flag", "workspace", "workspace_bytes", "rows", "n_state", "n_req",
                                                    "reserved0"]),
}


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
    for name in ENTRIES + ("tcavt_constraint_build", "tcavt_constraint_workspace_bytes"):
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.lib()
    assert lib.tcavt_constraint_workspace_bytes.restype is ctypes.c_int64
    assert list(lib.tcavt_constraint_build.argtypes) == [ctypes.POINTER(capi.ConstraintTable), ctypes.c_void_p]
    for name in ENTRIES:
        assert list(getattr(lib, name).argtypes) == [ctypes.POINTER(capi.ConstraintArgs), ctypes.c_void_p]
    assert lib.tcavt_abi_version() == capi.ABI_VERSION == 5  # no existing struct or entry changed


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_mirror_matches_header_layout(tmp_path, cname):
    cls, want = STRUCTS[cname]
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_] == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + f'  printf("%zu\\n", sizeof({cname}));\n'
                   + "".join(f'  printf("%zu\\n", offsetof({cname}, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(cls)
    assert out[1:] == [getattr(cls, n).offset for n in names]


def _table(V=1000, n_states=5, n_classes=7):
    """A table that passes every check (fake, 16-byte aligned pointers: a refusal never dereferences one)."""
    t = capi.ConstraintTable()
    for n in TABLE_POINTERS:
        setattr(t, n, 4096)
    t.V, t.n_states, t.n_classes = V, n_states, n_classes
    return t


def _valid(rows=3, form="batch", table=None):
    a = capi.ConstraintArgs()
    a._table = table if table is not None else _table()  # (kept alive with the struct)
    a.table = ctypes.pointer(a._table)
    for n in POINTERS:
        setattr(a, n, 4096)
    if form in ("slots", "rows"):
        a.out_row = 4096
    if form == "rows":
        a.slot_of_row, a.n_state = 4096, 4
    a.rows, a.n_req = rows, 8
    a.workspace_bytes = capi.lib().tcavt_constraint_workspace_bytes(rows)
    return a


def _refused(entry, a, *words):
    rc = getattr(capi.lib(), entry)(ctypes.byref(a) if a is not None else None, None)
    msg = capi.lib().tcavt_last_error()
    assert rc == 1, (entry, words, rc)
    assert entry[len("tcavt_"):].encode() in msg and all(w.encode() in msg for w in words), (entry, words, msg)


def _table_refusals(entry, wrap):
    """The refusals of the table, through ``entry``; wrap(table) makes the entry's argument."""
    for n in TABLE_POINTERS:
        t = _table()
        setattr(t, n, None)
        _refused(entry, wrap(t), f"table: {n} is a null pointer")
    for bad in (0, -1):
        t = _table(V=bad)
        _refused(entry, wrap(t), f"V = {bad}")
    for field in ("n_states", "n_classes"):
        for bad in (0, -1, 4097):
            t = _table()
            setattr(t, field, bad)
            _refused(entry, wrap(t), f"{field} = {bad}", "4096")
    t = _table()
    t.token_class = 4096 + 4
    _refused(entry, wrap(t), "token_class", "16-byte aligned")
    for n in ("trans", "bitmap", "count"):
        t = _table()
        setattr(t, n, 4096 + 2)
        _refused(entry, wrap(t), "4-byte aligned")
    t = _table(n_states=4096, n_classes=4096)  # the bounds themselves are legal: the next refusal is another one
    a = _valid(table=t)
    a.rows = 0
    _refused("tcavt_constraint_mask", a, "rows = 0")


def test_build_refuses_a_bad_table_without_a_device():
    _refused("tcavt_constraint_build", None, "table", "null pointer")
    _table_refusals("tcavt_constraint_build", lambda t: t)


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_refusal_is_reported_without_a_device(entry):
    _refused(entry, None, "args", "null pointer")
    a = _valid()
    a.table = None
    _refused(entry, a, "table is a null pointer")
    _table_refusals(entry, lambda t: _valid(table=t))
    for form in ("batch", "slots", "rows"):
        for n in POINTERS:
            a = _valid(form=form)
            setattr(a, n, None)
            _refused(entry, a, n + " is a null pointer")
    a = _valid(form="rows")
    a.out_row = None  # the rows form reads the request index at out_row[s]
    _refused(entry, a, "out_row is a null pointer")
    for n in ("rows", "n_req"):
        for bad in (0, -1):
            a = _valid(form="slots")
            setattr(a, n, bad)
            _refused(entry, a, f"{n} = {bad}")
    for bad in (0, -2):
        a = _valid(form="rows")
        a.n_state = bad
        _refused(entry, a, f"n_state = {bad}", "slot_of_row")
    a = _valid(rows=9)  # the batch form reads start[row]
    _refused(entry, a, "n_req = 8", "rows = 9", "batch form")
    a = _valid(rows=9, form="slots")
    a.rows = 0  # (the slots form takes n_req < rows: the next refusal is another one)
    _refused(entry, a, "rows = 0")
    for n in ("logits", "state", "start", "request_state", "flag"):
        a = _valid()
        setattr(a, n, 4096 + 2)
        _refused(entry, a, "4-byte aligned")
    a = _valid()
    a.workspace_bytes -= 1
    _refused(entry, a, "workspace_bytes")
    a = _valid()
    a.workspace = 4096 + 8
    _refused(entry, a, "workspace", "16-byte aligned")


def test_workspace_bytes_is_monotone_and_zero_without_rows():
    f = capi.lib().tcavt_constraint_workspace_bytes
    assert f(0) == 0 and f(-3) == 0
    prev = 0
    for rows in (1, 2, 3, 5, 8, 32, 33, 256):
        now = f(rows)
        assert now > prev and now % 16 == 0
        prev = now
