"""CPU-side checks of the decoder attention beyond 544 rows: tcavt_attn_causal_gqa_stream, tcavt_attn_bwd_stream and
tcavt_attn_bwd_stream_ok are exported and bound, the ABI version is unchanged, the dispatch predicates say what the header says,
and every argument error of the two entries is returned before anything touches a device (fake aligned pointers: a call that
got past its checks would dereference them)."""
import ctypes
import os
import re

import pytest

SCALE = 0.125
NEW = ("tcavt_attn_causal_gqa_stream", "tcavt_attn_bwd_stream", "tcavt_attn_bwd_stream_ok")


def _err():
    from tcavt_amd import capi

    return capi.lib().tcavt_last_error() or b""


def test_symbols_are_exported_and_bound():
    from tcavt_amd import capi, ops

    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(handle, name), name
        assert name in capi.EXPORTED_SYMBOLS, name
        assert getattr(capi.lib(), name).argtypes is not None, name
    assert callable(ops.attn_causal_gqa_stream) and callable(ops.attn_bwd_stream) and callable(ops.attn_bwd_stream_ok)
    assert ops.ATTN_STREAM_MAX_L == 2048 and ops.ATTN_RESIDENT_MAX_L == 544


def test_abi_version_is_still_5():
    from tcavt_amd import capi

    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tcavt.h")) as f:
        header = f.read()
    assert re.search(r"^#define TCAVT_ABI_VERSION 5$", header, re.M)
    assert re.search(r"^#define TCAVT_ATTN_STREAM_MAX_L 2048$", header, re.M)
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name


@pytest.mark.parametrize("T", [544, 545, 2048, 2049])
@pytest.mark.parametrize("group", [1, 3, 4, 16])
def test_stream_ok_truth_table(T, group):
    from tcavt_amd import capi, ops

    want = int(544 < T <= 2048 and 16 % group == 0)
    for nkv in (1, 2):
        assert capi.lib().tcavt_attn_bwd_stream_ok(T, group * nkv, nkv) == want, (T, group, nkv)
        assert ops.attn_bwd_stream_ok(T, group * nkv, nkv) is bool(want)


def test_long_ok_still_stops_at_544():
    from tcavt_amd import capi

    for nq, nkv in ((32, 8), (4, 4), (16, 1)):
        assert capi.lib().tcavt_attn_bwd_long_ok(544, nq, nkv) == 1
        assert capi.lib().tcavt_attn_bwd_long_ok(545, nq, nkv) == 0
    assert capi.lib().tcavt_attn_bwd_stream_ok(545, 5, 2) == 0 and capi.lib().tcavt_attn_bwd_stream_ok(545, 4, 0) == 0
    # the existing entries keep refusing 545 (fake pointers: refused before any launch)
    rc = capi.lib().tcavt_attn_bwd_long(*([64] * 9), 1, 545, 4, 1, 64, SCALE, capi.F16, None)
    assert rc == 1 and b"attn_bwd_long:" in _err() and b"outside the chunked form" in _err()
    rc = capi.lib().tcavt_attn_causal_gqa_lse(64, 64, 64, 64, 1, 545, 4, 1, SCALE, capi.F16, None)
    assert rc == 1 and b"attn_causal_gqa: L=545" in _err()


def test_forward_argument_errors_before_any_launch():
    from tcavt_amd import capi

    f = capi.lib().tcavt_attn_causal_gqa_stream

    def call(qkv=64, out=64, lse=64, kv=64, B=1, L=600, nq=4, nkv=1, dt=None):
        return f(qkv, out, lse, kv, B, L, nq, nkv, SCALE, capi.F16 if dt is None else dt, None)

    cases = [("null qkv", dict(qkv=None), b"null pointer"), ("null out", dict(out=None), b"null pointer"),
             ("null kv_len", dict(kv=None), b"null pointer"), ("L = 0", dict(L=0), b"L=0"), ("L = 2049", dict(L=2049), b"L=2049"),
             ("B = 0", dict(B=0), b"must be in"), ("group 9", dict(nq=9), b"nq/nkv"), ("nq % nkv", dict(nq=5, nkv=2), b"nq/nkv"),
             ("nkv = 0", dict(nkv=0), b"nq/nkv"), ("f32", dict(dt=capi.F32), b"dtype16"),
             ("misaligned qkv", dict(qkv=72), b"unaligned"), ("misaligned out", dict(out=72), b"unaligned")]
    for name, kw, frag in cases:
        capi.lib().tcavt_attn_bwd_long_ok(0, 0, 0)  # (something else in between: the message below is this call's own)
        rc = call(**kw)
        assert rc == 1, name
        assert _err().startswith(b"attn_causal_gqa_stream:") and frag in _err(), (name, _err())


def test_backward_argument_errors_before_any_launch():
    from tcavt_amd import capi

    f = capi.lib().tcavt_attn_bwd_stream
    ok = [64] * 9  # (non-null, 16-byte aligned; never dereferenced: every call below is refused)

    def call(ptrs=ok, B=1, T=600, nq=4, nkv=1, hd=64, dt=None):
        return f(*ptrs, B, T, nq, nkv, hd, SCALE, capi.F16 if dt is None else dt, None)

    for i in range(9):
        a = list(ok)
        a[i] = None
        assert call(ptrs=a) == 1 and _err().startswith(b"attn_bwd_stream:") and b"bad args" in _err(), i
    for i in (0, 1, 2, 4, 5):  # qkv, dO, att, g_qkv, stats
        a = list(ok)
        a[i] = 72
        assert call(ptrs=a) == 1 and _err().startswith(b"attn_bwd_stream:") and b"alignment" in _err(), i
    for name, kw, frag in (("T = 0", dict(T=0), b"bad args"), ("T = 2049", dict(T=2049), b"outside the chunked form"),
                           ("group 3", dict(nq=3), b"outside the chunked form"), ("group 32", dict(nq=32), b"outside the chunked form"),
                           ("head_dim 32", dict(hd=32), b"head_dim"), ("nq % nkv", dict(nq=5, nkv=2), b"head_dim"),
                           ("f32", dict(dt=capi.F32), b"bad args"), ("B = 0", dict(B=0), b"bad args")):
        assert call(**kw) == 1, name
        assert _err().startswith(b"attn_bwd_stream:") and frag in _err(), (name, _err())
    assert b"T <= 2048" in (call(T=2049), _err())[1]


def test_stack_forward_refuses_past_the_cap_before_any_launch():
    from tcavt_amd import capi

    a = capi.LlamaStackArgs()
    for k in ("layers", "gamma_final", "rope_cos", "rope_sin", "h16", "part", "kv_len", "att", "act", "out16"):
        fld = dict(capi.LlamaStackArgs._fields_)[k]
        setattr(a, k, ctypes.cast(64, fld) if fld is not ctypes.c_void_p else 64)
    a.n_layers, a.B, a.L, a.H, a.I, a.nq, a.nkv, a.dtype16 = 1, 1, 2049, 256, 256, 4, 1, capi.F16
    rc = capi.lib().tcavt_llama_stack_forward(ctypes.byref(a), None)
    assert rc == 1 and b"llama_stack_forward: L=2049" in _err(), _err()
