"""quant.py, the plain-torch definition of the decode step's FP8 weight format (include/tcavt.h: tcavt_pack_weight8): e4m3fn
codes of each row times a power of two, the smallest that brings the row's largest magnitude to <= 448.  Everything here is
exact: a power-of-two scale costs a floating-point format no precision, so every check is an equality."""
import pytest
import torch

DTYPES = [torch.float16, torch.bfloat16]


def _next_up(x):
    """The next 16-bit value above x > 0 (same type)."""
    return (x.view(torch.int16) + 1).view(x.dtype)


def _matrix(dt, N=48, K=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-6, 3, (N, 1), generator=g).float())
    return w.to(dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_row_exponent_is_minimal_at_the_scale_boundaries(dt):
    """amax = 448 * 2^j fits at k = j exactly; the next 16-bit value above it needs k = j + 1.  An all-zero row has k = 0."""
    from tcavt_amd import quant

    js = list(range(-14, 7))  # 448 * 2^j: normal in fp16 from j = -14 (2^-6 * 1.75) up to 448 * 64 = 28672
    on = torch.tensor([448.0 * 2.0 ** j for j in js]).to(dt)
    assert torch.equal(on.double(), torch.tensor([448.0 * 2.0 ** j for j in js], dtype=torch.float64))
    w = torch.zeros(2 * len(js) + 1, 32, dtype=dt)
    w[: len(js), 3] = -on                       # the sign plays no part
    w[len(js): 2 * len(js), 17] = _next_up(on)
    w[:, 0] = torch.tensor(2.0 ** -14).to(dt)   # something small in every row but the last
    w[-1] = 0
    k = quant.row_exponents(w)
    assert k[: len(js)].tolist() == js
    assert k[len(js): 2 * len(js)].tolist() == [j + 1 for j in js]
    assert k[-1].item() == 0
    # minimal: the scaled maximum is <= 448, and one binade further down it would not be
    amax = w.double().abs().amax(dim=1)[:-1]
    kk = k[:-1].double()
    assert (amax * torch.exp2(-kk) <= 448).all() and (amax * torch.exp2(-(kk - 1)) > 448).all()
    codes, _ = quant.quantize(w)
    assert codes[-1].eq(0).all() and torch.equal(quant.scales(k).double(), torch.exp2(k.double()))


@pytest.mark.parametrize("dt", DTYPES)
def test_codes_are_torch_e4m3fn_of_the_scaled_rows(dt):
    """Byte for byte (w * 2^-k).to(float8_e4m3fn): round to nearest even, subnormals included.  Checked on random rows and
    on planted values: exact ties between neighbouring codes and values in the subnormal range of e4m3."""
    from tcavt_amd import quant

    w = _matrix(dt, seed=1)
    w[:, 0] = 256.0                                                  # k = 0 in every row: the values below are what is encoded
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, 25.0, 27.0, 29.0, 31.0, 34.0, 38.0, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10,
                         2.0 ** -9, 2.0 ** -8, 7 * 2.0 ** -9, 15 * 2.0 ** -10, 2.0 ** -6, 2.0 ** -11, -17.0, -2.0 ** -10])
    w[5, 1:1 + len(ties)] = ties.to(dt)
    assert torch.equal(w[5, 1:1 + len(ties)].float(), ties)
    codes, k = quant.quantize(w)
    assert k.eq(0).all()
    want = w.float().to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want)
    got = codes[5, 1:1 + len(ties)].view(torch.float8_e4m3fn).float()
    # ties go to the even code: 17 -> 16, 19 -> 20, ..., 2^-10 (half the smallest subnormal) -> 0, 3 * 2^-10 -> 2^-8
    assert got[:4].tolist() == [16.0, 20.0, 20.0, 24.0] and got[10].item() == 0.0 and got[11].item() == 2.0 ** -8
    assert got[12].item() == 2.0 ** -8 and got[16].item() == 2.0 ** -6 and got[18].item() == 0.0 and got[19].item() == -16.0
    # general rows: the same identity with the row's own scale
    w = _matrix(dt, seed=2)
    codes, k = quant.quantize(w)
    want = torch.ldexp(w.float(), -k[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(codes, want) and len(set(k.tolist())) > 3


@pytest.mark.parametrize("dt", DTYPES)
def test_round_trip_is_lossless_the_second_time(dt):
    """dequantize(quantize(w)) is a fixed point: quantising it again returns the same matrix -- also where the second k is
    smaller than the first because the row's maximum was rounded down across a scale boundary."""
    from tcavt_amd import quant

    w = _matrix(dt, seed=3)
    # row 7: amax just above 448 * 2^-3 -> k = -2, where it rounds DOWN to 224 * 2^-2 = 448 * 2^-3: the second k is -3
    w[7] = (w[7].float().clamp(-20, 20)).to(dt)
    w[7, 9] = _next_up(torch.tensor(56.0).to(dt))
    c1, k1 = quant.quantize(w)
    d1 = quant.dequantize(c1, k1, dt)
    c2, k2 = quant.quantize(d1)
    d2 = quant.dequantize(c2, k2, dt)
    assert k1[7].item() == -2 and k2[7].item() == -3 and (k2 <= k1).all()
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))
    # the dequantised values are what the codes say, exactly, and within half an e4m3 step (2^-4 relative) of w
    assert torch.equal(d1.double(), c1.view(torch.float8_e4m3fn).double() * torch.exp2(k1.double())[:, None])
    big = w.double().abs() >= torch.exp2(k1.double() - 6)[:, None]  # (scaled magnitude in e4m3's normal range)
    assert ((d1.double() - w.double()).abs()[big] <= w.double().abs()[big] * 2.0 ** -4).all()
    assert torch.equal(quant.snap(quant.snap(w)).view(torch.int16), quant.snap(w).view(torch.int16))


def test_pack_and_unpack_are_inverses_and_follow_the_lane_order():
    from tcavt_amd import quant

    N, K = 48, 1280
    codes = torch.randint(0, 256, (N, K), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    flat = quant.pack_chunks(codes)
    assert flat.shape == (N * K,) and torch.equal(quant.unpack_chunks(flat, N, K), codes)
    assert torch.equal(quant.pack_chunks(quant.unpack_chunks(flat, N, K)), flat)
    for b, j, l in ((0, 0, 0), (1, 3, 17), (2, 39, 63), (0, 5, 40)):
        q, r = l >> 4, l & 15
        off = (b * (K // 32) + j) * 512 + 8 * l
        assert torch.equal(flat[off:off + 8], codes[16 * b + r, 32 * j + 8 * q: 32 * j + 8 * q + 8])


@pytest.mark.parametrize("dt", DTYPES)
def test_whole_buffer_and_non_finite_rows(dt):
    """pack(w): N * K code bytes, then N fp32 scales, each exactly 2^k; unpack returns codes and k.  A row with an inf or a
    NaN: the NaN code everywhere, scale 1."""
    from tcavt_amd import quant

    w = _matrix(dt, seed=5)
    w[3, 100] = float("inf")
    w[20, 0] = float("nan")
    N, K = w.shape
    buf = quant.pack(w)
    assert buf.dtype == torch.uint8 and buf.numel() == N * K + 4 * N
    codes, k = quant.unpack(buf, N, K)
    c0, k0 = quant.quantize(w)
    assert torch.equal(codes, c0) and torch.equal(k, k0)
    assert codes[3].eq(0x7F).all() and codes[20].eq(0x7F).all() and k[3].item() == 0 and k[20].item() == 0
    sc = buf[N * K:].view(torch.float32)
    assert torch.equal(sc.double(), torch.exp2(k.double()))
    d = quant.dequantize(codes, k, dt)
    assert torch.isnan(d[3]).all() and torch.isnan(d[20]).all() and torch.isfinite(d[[0, 1, 2, 4]].float()).all()
