"""quant.py's MX8 format (OCP MXFP8-E4M3 with the project's scale rule) on the CPU: the definition the kernels are tested against."""
import pytest
import torch

from tcavt_amd import quant

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])


def _lut():
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()


def _wide(dt, R=24, K=256, seed=0):
    """values over the whole exponent range of dt, both signs, zeros sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    emin, emax = (-24, 15) if dt == F16 else (-133, 127)
    e = torch.randint(emin, emax + 1, (R, K // 32, 1), generator=g) + torch.randint(-6, 1, (R, K // 32, 32), generator=g)
    x = torch.ldexp(torch.randn(R, K // 32, 32, generator=g).double(), e.clamp(emin, emax).to(torch.int32)).reshape(R, K)
    x[torch.rand(R, K, generator=g) < 0.05] = 0.0
    x = x.to(dt)
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


@DTYPES
def test_dequantize_of_quantize_is_snap_and_snap_is_idempotent(dt):
    x = torch.cat([_wide(dt), (torch.randn(8, 256, generator=torch.Generator().manual_seed(1)) * 3).to(dt)])
    codes, sb = quant.quantize_mx(x)
    assert codes.dtype == sb.dtype == torch.uint8 and codes.shape == x.shape and sb.shape == (x.shape[0], x.shape[1] // 32)
    assert int(sb.max()) <= 254  # (uint8: >= 0 by type)
    xq = quant.dequantize_mx(codes, sb, dt)
    if dt == F16:  # snap drops what is below the smallest fp16 normal, nothing else
        xq = torch.where(xq.abs() < 2.0 ** -14, torch.zeros_like(xq), xq)
    s = quant.snap_mx(x)
    assert torch.equal(s.view(torch.int16), xq.view(torch.int16))
    assert torch.equal(quant.snap_mx(s).view(torch.int16), s.view(torch.int16))
    # float64 dequantisation is exact: code value times 2^k, and never further from x than half an e4m3 step of the block
    d64 = quant.dequantize_mx(codes, sb, torch.float64)
    k = sb.to(torch.int32) - 127
    assert torch.equal(d64, torch.ldexp(_lut()[codes.long()].view(x.shape[0], -1, 32), k[:, :, None]).view(x.shape))
    step = torch.ldexp(torch.full_like(d64, 16.0).view(x.shape[0], -1, 32), k[:, :, None]).view(x.shape)  # half of the largest step (32)
    assert ((d64 - x.double()).abs() <= step).all()
    # the scaled block fits e4m3 and k is minimal (unless clamped)
    amax = x.double().abs().view(x.shape[0], -1, 32).amax(-1)
    nz = amax > 0
    assert (torch.ldexp(amax, -k)[nz] <= 448).all()
    assert ((torch.ldexp(amax, -(k - 1)) > 448) | (k == -127))[nz].all()


@DTYPES
def test_block_amax_at_448_times_a_power_of_two_and_one_ulp_above(dt):
    ulp = 2.0 ** -2 if dt == F16 else 2.0  # of dt at 448 = 1.75 * 2^8
    for j in (-20, -3, 0, 5) + ((60, 100) if dt == BF16 else ()):
        x = torch.zeros(2, 64, dtype=torch.float64)
        x[0, 5] = -448.0 * 2.0 ** j                       # exactly the largest e4m3 value at k = j
        x[0, 6] = 17.0 * 2.0 ** j
        x[1, 40] = (448.0 + ulp) * 2.0 ** j               # one ulp of dt above: k = j + 1
        x[1, 41] = 448.0 * 2.0 ** j
        xt = x.to(dt)
        assert torch.equal(xt.double(), x)
        codes, sb = quant.quantize_mx(xt)
        assert sb.tolist() == [[127 + j, 127], [127, 127 + j + 1]]
        assert codes[0, 5] == 0xFE and codes[1, 40] == 0x76  # -448; 224 (448 (1 + ulp) / 2 rounds down to 224)
        assert codes[1, 41] == 0x76                          # 448 / 2, exact
        assert codes[0, 6] == 0x58                           # 17 is half-way between 16 and 18: ties to even -> 16


@DTYPES
def test_zero_and_nonfinite_blocks(dt):
    x = torch.ones(3, 96, dtype=dt)
    x[0, 32:64] = 0
    x[0, 40] = -0.0
    x[1, 95] = float("inf")
    x[2, 0] = float("nan")
    x[2, 64] = -float("inf")
    codes, sb = quant.quantize_mx(x)
    assert sb[0].tolist() == [119, 127, 119] and codes[0, 32:64].tolist() == [0] * 8 + [0x80] + [0] * 23
    assert sb[1].tolist() == [119, 119, 127] and (codes[1, 64:] == 0x7F).all() and (codes[1, :64] == 0x78).all()  # 1 * 2^8 = 256
    assert sb[2].tolist() == [127, 119, 127] and (codes[2, :32] == 0x7F).all() and (codes[2, 64:] == 0x7F).all()
    d = quant.dequantize_mx(codes, sb, torch.float64)
    assert torch.isnan(d[1, 64:]).all() and torch.isnan(d[2, :32]).all() and torch.equal(d[0, :32], torch.ones(32, dtype=torch.float64))


def test_ones_scale():
    """1.0 = 0.5 * 2^1: k = 1 - 9 = -8, code = 256 -> 0x78"""
    codes, sb = quant.quantize_mx(torch.ones(1, 32, dtype=F16))
    assert sb.tolist() == [[119]] and (codes == 0x78).all()


def test_fp16_subnormals():
    x = torch.zeros(1, 64, dtype=F16)
    x[0, 3] = 2.0 ** -24          # the smallest fp16 subnormal alone in its block: k = -32, code = 256
    x[0, 32] = 2.0 ** -15         # subnormal next to a normal number
    x[0, 33] = 3 * 2.0 ** -24
    x[0, 34] = 1.0
    codes, sb = quant.quantize_mx(x)
    assert sb.tolist() == [[127 - 32, 119]]
    assert codes[0, 3] == 0x78
    d = quant.dequantize_mx(codes, sb, torch.float64)
    assert d[0, 3] == 2.0 ** -24 and d[0, 32] == 2.0 ** -15 and d[0, 34] == 1.0
    assert codes[0, 33] == 0 and d[0, 33] == 0  # 3 * 2^-24 * 2^8 is 0.023 of the smallest e4m3 step (2^-9): underflows
    assert torch.equal(quant.snap_mx(x)[0, :32], torch.zeros(32, dtype=F16))  # snap drops fp16 subnormals


def test_bf16_block_below_the_clamp():
    x = torch.zeros(1, 64, dtype=BF16)
    x[0, 0] = 2.0 ** -130
    x[0, 1] = -(2.0 ** -133)     # the smallest bf16 subnormal
    x[0, 32] = 2.0 ** -100
    codes, sb = quant.quantize_mx(x)
    assert sb.tolist() == [[0, 127 - 108]]  # first block clamped to k = -127 (the rule alone gives -138)
    assert codes[0, 0] == 0x20 and codes[0, 1] == 0x88  # 2^-3 and -2^-6 (the smallest normal code)
    d = quant.dequantize_mx(codes, sb, torch.float64)
    assert d[0, 0] == 2.0 ** -130 and d[0, 1] == -(2.0 ** -133) and d[0, 32] == 2.0 ** -100 and codes[0, 32] == 0x78


def test_ties_to_even_on_half_way_values():
    """block amax 448 (k = 0): every value half-way between two neighbouring e4m3 numbers goes to the even mantissa"""
    lut = _lut()
    pos = lut[:0x7F]  # 0 .. 448, ascending
    mid = (pos[:-1] + pos[1:]) / 2
    ok = mid.to(BF16).double() == mid
    mid, lo = mid[ok], torch.arange(0x7E)[ok]
    assert len(mid) >= 100
    for sign in (1.0, -1.0):
        x = torch.zeros(len(mid), 32, dtype=torch.float64)
        x[:, 0] = 448.0
        x[:, 1] = sign * mid
        codes, sb = quant.quantize_mx(x.to(BF16))
        assert (sb == 127).all()
        want = torch.where(lo % 2 == 0, lo, lo + 1) | (0x80 if sign < 0 else 0)
        assert torch.equal(codes[:, 1].long(), want)


def test_shape_and_dtype_are_checked():
    with pytest.raises(AssertionError):
        quant.quantize_mx(torch.zeros(2, 48, dtype=F16))
    with pytest.raises(AssertionError):
        quant.quantize_mx(torch.zeros(2, 64))
