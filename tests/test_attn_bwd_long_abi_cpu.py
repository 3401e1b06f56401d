"""CPU-side checks of the chunked attention backward's boundary (tcavt_attn_bwd_long / tcavt_attn_bwd_long_ok: exported,
bound, refusing bad arguments before anything touches a device) and of custom_collate_fn(pad_to_multiple_of=...)."""
import ctypes

import pytest
import torch


def test_symbols_are_exported_and_bound():
    from tcavt_amd import capi, ops

    handle = ctypes.CDLL(capi.LIB_PATH)
    for name in ("tcavt_attn_bwd_long", "tcavt_attn_bwd_long_ok"):
        assert hasattr(handle, name), name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert callable(ops.attn_bwd_long) and callable(ops.attn_bwd_long_ok)
    assert capi.lib().tcavt_abi_version() == capi.ABI_VERSION == 5


@pytest.mark.parametrize("T,nq,nkv,want", [(256, 32, 8, 0), (257, 32, 8, 1), (544, 32, 8, 1), (545, 32, 8, 0), (300, 12, 4, 0),
                                           (300, 4, 4, 1)])
def test_long_ok(T, nq, nkv, want):
    from tcavt_amd import capi, ops

    assert capi.lib().tcavt_attn_bwd_long_ok(T, nq, nkv) == want
    assert ops.attn_bwd_long_ok(T, nq, nkv) is bool(want)


def test_resident_ok_is_unchanged():
    from tcavt_amd import capi

    assert capi.lib().tcavt_attn_bwd_resident_ok(256, 32, 8) == 1
    assert capi.lib().tcavt_attn_bwd_resident_ok(257, 32, 8) == 0


def test_argument_errors_are_reported_before_any_launch():
    from tcavt_amd import capi

    f = capi.lib().tcavt_attn_bwd_long
    ok = [64] * 9  # (non-null, 16-byte aligned; never dereferenced: every call below is refused)
    rc = f(*ok, 1, 545, 4, 1, 64, 0.125, capi.F16, None)
    assert rc == 1 and b"outside the chunked form" in capi.lib().tcavt_last_error()
    for i in range(9):
        a = list(ok)
        a[i] = None
        rc = f(*a, 1, 300, 4, 1, 64, 0.125, capi.F16, None)
        assert rc == 1 and b"attn_bwd_long" in capi.lib().tcavt_last_error(), i
    rc = f(*ok, 1, 300, 4, 1, 128, 0.125, capi.F16, None)
    assert rc == 1 and b"head_dim" in capi.lib().tcavt_last_error()
    rc = f(*ok, 1, 300, 12, 4, 64, 0.125, capi.F16, None)
    assert rc == 1 and b"outside the chunked form" in capi.lib().tcavt_last_error()
    a = list(ok)
    a[0] = 72
    rc = f(*a, 1, 300, 4, 1, 64, 0.125, capi.F16, None)
    assert rc == 1 and b"alignment" in capi.lib().tcavt_last_error()


def _items(lens):
    g = torch.Generator().manual_seed(3)
    out = []
    for i, n in enumerate(lens):
        out.append({
            "traj_emb": torch.randn(6, 2, generator=g), "target_traj": torch.randn(12, 2, generator=g),
            "vision_emb": torch.randn(4, 8, generator=g), "lane_polygon": torch.randn(5, 2, generator=g),
            "lane_polygon_len": 5 - i, "norm_stat": [0.0, 1.0, 2.0, 3.0], "context_str": f"c{i}", "answer_str": f"a{i}",
            "track_id": i, "input_ids": torch.randint(1, 100, (n,), generator=g), "attention_mask": torch.ones(n, dtype=torch.int64),
            "labels": torch.randint(1, 100, (n,), generator=g),
        })
    return out


def test_collate_pads_the_text_to_a_multiple():
    from tcavt_amd.data import custom_collate_fn

    lens = [13, 21, 5]
    batch = _items(lens)
    base = custom_collate_fn(batch)
    same = custom_collate_fn(batch, pad_to_multiple_of=None)
    assert list(base) == list(same)
    for k in base:
        if torch.is_tensor(base[k]):
            assert base[k].dtype == same[k].dtype and torch.equal(base[k], same[k]), k
        else:
            assert base[k] == same[k], k
    assert base["input_ids"].shape == (3, 21)
    pad = custom_collate_fn(batch, pad_to_multiple_of=8)
    for k, v in (("input_ids", 0), ("attention_mask", 0), ("labels", -100)):
        assert pad[k].shape == (3, 24) and pad[k].dtype == base[k].dtype, k
        assert torch.equal(pad[k][:, :21], base[k]), k
        assert (pad[k][:, 21:] == v).all(), k
        for b, n in enumerate(lens):
            assert (pad[k][b, n:] == v).all(), (k, b)
    for k in base:
        if k not in ("input_ids", "attention_mask", "labels"):
            assert torch.equal(pad[k], base[k]) if torch.is_tensor(base[k]) else pad[k] == base[k], k
    # already a multiple: nothing is added
    again = custom_collate_fn(_items([16, 3]), pad_to_multiple_of=8)
    assert again["input_ids"].shape == (2, 16)
    with pytest.raises(ValueError):
        custom_collate_fn(batch, pad_to_multiple_of=0)
