"""The C boundary of per-request sampling parameters (tcavt_sample_tokens_per_request, tcavt_request_params_check) -- no GPU: the
symbols are declared, exported and bound, the ABI version is unchanged, the ctypes mirror of tcavt_request_params has the header's
layout (through the host C compiler), the host check accepts good tables and names the failing index and field of a bad one, and
the launch entry reports every documented refusal before a device is touched."""
import ctypes
import os
import re
import subprocess

import pytest

from tcavt_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, CHECK = "tcavt_sample_tokens_per_request", "tcavt_request_params_check"
PAD = 7


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


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tcavt.h")).read()
    assert re.search(r"\bint\s+tcavt_sample_tokens_per_request\s*\(\s*const\s+tcavt_sample_args\s*\*\s*\w+\s*,\s*const\s+tcavt_request_params\s*\*"
                     r"\s*\w+\s*,\s*tcavt_stream_t\s+\w+\s*\)\s*;", header)
    assert re.search(r"\bint\s+tcavt_request_params_check\s*\(\s*const\s+tcavt_sample_params\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", header)
    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in (ENTRY, CHECK):
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in capi.EXPORTED_SYMBOLS
    lib = capi.lib()
    assert list(getattr(lib, ENTRY).argtypes) == [ctypes.POINTER(capi.SampleArgs), ctypes.POINTER(capi.RequestParams), ctypes.c_void_p]
    assert list(getattr(lib, CHECK).argtypes) == [ctypes.POINTER(capi.SampleParams), ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert lib.tcavt_abi_version() == capi.ABI_VERSION == 5  # additive: no existing struct or entry changed
    assert re.search(r"#define\s+TCAVT_ABI_VERSION\s+5\b", header)


def test_struct_mirror_matches_header_layout(tmp_path):
    cname, cls = "tcavt_request_params", capi.RequestParams
    names = _struct_fields(cname)
    assert names == [f[0] for f in cls._fields_]
    assert names == ["table", "min_new_tokens", "bad_index_flag", "n_req", "reserved0"]
    pname, pcls = "tcavt_sample_params", capi.SampleParams  # (the table's element: its layout is what the kernel reads)
    pnames = _struct_fields(pname)
    assert pnames == [f[0] for f in pcls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tcavt.h"\nint main(void) {\n'
                   + "".join(f'  printf("%zu\\n", sizeof({c}));\n' + "".join(f'  printf("%zu\\n", offsetof({c}, {n}));\n' for n in ns)
                             for c, ns in ((cname, names), (pname, pnames))) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    k = 1 + len(names)
    assert out[0] == ctypes.sizeof(cls) and out[1:k] == [getattr(cls, n).offset for n in names]
    assert out[k] == ctypes.sizeof(pcls) == 48 and out[k + 1:] == [getattr(pcls, n).offset for n in pnames]


# ---- tcavt_request_params_check (host only)
def _entry(**kw):
    d = dict(temperature=0.9, top_p=0.9, repetition_penalty=1.2, top_k=40, no_repeat_ngram_size=3, do_sample=1, eos_token_id=2,
             pad_token_id=PAD, seed=1)
    d.update(kw)
    return capi.SampleParams(d["temperature"], d["top_p"], d["repetition_penalty"], d["top_k"], d["no_repeat_ngram_size"], d["do_sample"],
                             d["eos_token_id"], d["pad_token_id"], d["seed"])


def _check(entries, mins=None, has_bitmap=0, n=None):
    table = (capi.SampleParams * len(entries))(*entries) if entries else None
    m = None if mins is None else (ctypes.c_int32 * len(mins))(*mins)
    rc = capi.lib().tcavt_request_params_check(table, m, len(entries) if n is None else n, has_bitmap)
    return rc, capi.lib().tcavt_last_error()


def test_check_accepts_good_tables():
    good = [_entry(), _entry(do_sample=0, temperature=0.0, top_k=0, top_p=0.0),  # (greedy: the warpers' values are not looked at)
            _entry(top_k=1, top_p=1.0, temperature=1e-3), _entry(top_k=256, eos_token_id=-1, seed=(1 << 63) + 5),
            _entry(repetition_penalty=1.0, no_repeat_ngram_size=0)]
    assert _check(good)[0] == 0
    assert _check(good, mins=[0, 3, 1, 0, 7])[0] == 0            # entry 3 has no EOS, and no minimum
    assert _check(good, mins=[0, 3, 1, 2, 7], has_bitmap=1)[0] == 0  # ... or a stop set to ban
    assert _check([_entry()], mins=[5])[0] == 0


BAD_FIELDS = [("temperature", 0.0), ("temperature", -1.0), ("top_k", 0), ("top_k", 257), ("top_p", 0.0), ("top_p", 1.5),
              ("repetition_penalty", 0.0), ("repetition_penalty", -2.0), ("no_repeat_ngram_size", -1)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
@pytest.mark.parametrize("index", [0, 3])
def test_check_names_the_failing_index_and_field(field, value, index):
    entries = [_entry(seed=i) for i in range(5)]
    entries[index] = _entry(**{field: value})
    rc, msg = _check(entries, mins=[0] * 5)
    assert rc == 1 and msg.startswith(b"request_params_check:"), (rc, msg)
    assert b"table[%d].%s" % (index, field.encode()) in msg, msg


def test_check_of_the_minimum_the_pad_and_the_arguments():
    entries = [_entry(seed=i) for i in range(4)]
    rc, msg = _check(entries, mins=[0, 0, -1, 0])
    assert rc == 1 and b"min_new_tokens[2] = -1" in msg, msg
    entries[1] = _entry(eos_token_id=-1)
    rc, msg = _check(entries, mins=[1, 2, 1, 1])  # a positive minimum with nothing to ban
    assert rc == 1 and b"min_new_tokens[1] = 2" in msg and b"eos_token_id" in msg and b"nothing to ban" in msg, msg
    assert _check(entries, mins=[1, 2, 1, 1], has_bitmap=1)[0] == 0
    assert _check(entries, mins=[1, 0, 1, 1])[0] == 0
    assert _check(entries)[0] == 0  # (no minima: nothing to ban is no error)
    entries[3] = _entry(pad_token_id=PAD + 1)
    rc, msg = _check(entries)
    assert rc == 1 and b"table[3].pad_token_id" in msg and b"table[0].pad_token_id" in msg, msg
    rc, msg = _check([], n=3)
    assert rc == 1 and b"host_table" in msg and b"null pointer" in msg, msg
    for n in (0, -2):
        rc, msg = _check([_entry()], n=n)
        assert rc == 1 and b"n_req = %d" % n in msg, msg
    greedy_bad = _entry(do_sample=0, repetition_penalty=0.0)  # (the processors' values count for greedy rows too)
    rc, msg = _check([_entry(), greedy_bad])
    assert rc == 1 and b"table[1].repetition_penalty" in msg, msg


# ---- the launch entry's refusals (no device: a refusal never dereferences a pointer)
POINTERS = ("logits", "history", "hist_len", "step", "cur_tok", "pos", "finished", "out_tokens")


def _valid(form="batch", rows=3):
    sp = _entry()
    a = capi.SampleArgs()
    for n in POINTERS:
        setattr(a, n, 4096)
    a.params = ctypes.pointer(sp)
    if form in ("slots", "rows"):
        a.max_new = a.out_row = 4096
    if form == "rows":
        a.slot_of_row, a.n_state = 4096, 4
    a.rows, a.V, a.hist_cap, a.out_cap = rows, 1000, 40, 8
    r = capi.RequestParams()
    r.table, r.n_req = ctypes.cast(4096, ctypes.POINTER(capi.SampleParams)), 5
    return a, r, sp


def _refused(a, r, *words):
    lib = capi.lib()
    rc = lib.tcavt_sample_tokens_per_request(ctypes.byref(a) if a is not None else None, ctypes.byref(r) if r is not None else None, None)
    msg = lib.tcavt_last_error()
    assert rc == 1 and msg.startswith(b"sample_tokens_per_request:") and all(w.encode() in msg for w in words), (words, rc, msg)


def test_the_launch_entry_refuses_bad_arguments_without_a_device():
    a, r, _sp = _valid()
    _refused(None, r, "args", "null pointer")
    _refused(a, None, "request params", "null pointer")
    for form in ("batch", "slots", "rows"):
        a, r, _sp = _valid(form)
        r.table = None
        _refused(a, r, "table is a null pointer")
        for n in (0, -1):
            a, r, _sp = _valid(form)
            r.n_req = n
            _refused(a, r, f"n_req = {n}")
        # the pointer rules of the form, as in tcavt_sample_tokens
        for n in POINTERS + ("params",) + (("max_new", "out_row") if form != "batch" else ()):
            a, r, _sp = _valid(form)
            setattr(a, n, None)
            if form == "slots" and n in ("max_new", "out_row"):
                pass  # (the other of the two still makes it the slots form)
            _refused(a, r, f"{n} is a null pointer")
        for n in ("rows", "V", "hist_cap", "out_cap"):
            a, r, _sp = _valid(form)
            setattr(a, n, 0)
            _refused(a, r, f"{n} = 0")
    a, r, _sp = _valid("rows")
    a.n_state = 0
    _refused(a, r, "n_state = 0", "slot_of_row")
    a, r, _sp = _valid("batch", rows=6)  # the request of row b is b: the table must cover the rows
    _refused(a, r, "n_req = 5", "rows = 6")
    a, r, _sp = _valid("slots", rows=6)  # (slots: any n_req >= 1; the kernel checks out_row[s]) -- passes the checks up to the launch
    for field, value, word in (("table", 4096 + 4, "table must be 8-byte aligned"), ("min_new_tokens", 4096 + 2, "min_new_tokens must be 4-byte aligned"),
                               ("bad_index_flag", 4096 + 1, "bad_index_flag must be 4-byte aligned")):
        a, r, _sp = _valid("slots")
        if field == "table":
            r.table = ctypes.cast(value, ctypes.POINTER(capi.SampleParams))
        else:
            setattr(r, field, value)
        _refused(a, r, word)
    # the ending rules are checked as in tcavt_sample_tokens
    a, r, _sp = _valid("slots")
    rules = capi.StopRules()
    rules.n_seqs = 17
    a.stop = ctypes.pointer(rules)
    _refused(a, r, "n_seqs = 17")
    # ... and so is the call's own struct
    a, r, sp = _valid("slots")
    sp.top_k = 0
    _refused(a, r, "top_k")
