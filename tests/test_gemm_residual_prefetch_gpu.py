"""The 16-bit residual stream epilogue of the 4-wave GEMM (tile codes 257 and 272) with its residual tile prefetched by LDS-DMA.

With TCAVT_EPI_RESIDUAL on the 16-bit stream (NORM_OUT, C == NULL) a workgroup's look-ahead past the last K-tile of its last
output tile carries that tile's residual into the two LDS tile buffers, and the epilogue reads it there (csrc/gemm_w4.hpp).
TCAVT_GEMM_NO_RES_PREFETCH=1, read at every launch, keeps the global loads in the epilogue.  test_gemm_forms_gpu.py covers both
tile codes at K = 128 and 256; here are the shapes where the prefetch itself can go wrong:

- buffer parity and short loops: K = 64 (one K-tile: both halves are issued around a single loop pass), 128, 192, 256, 320 (odd
  and even K-tile counts: the buffer that holds each residual half flips), tile 272 also at K = 4096 (the smallest K the
  dispatcher picks it for by itself); M = N = 256 (one workgroup) and 512 (four);
- the stream modes: in place, out of place (source bit-unchanged), norm_scale = 2^-3, and no residual (nothing is prefetched),
  fp16 and bf16, ldc = N + 16 with NaN padding and NaN rows that must stay as they are;
- a persistent launch with two kinds of workgroups: 264 tiles on 256 CUs, eight workgroups take the epilogue with global loads
  for their first tile and the prefetch for their last;
- a +-inf residual element must raise the non-finite flag through LDS as it does through registers.

Every call is checked against float64 (bit for bit in the exact regime, the per-element bound of test_gemm_forms_gpu.py
otherwise) AND, bit for bit, against the same call under TCAVT_GEMM_NO_RES_PREFETCH=1 in the same process.
"""
import contextlib
import os

import pytest
import torch

from test_gemm_forms_gpu import BF16, F16, F32, U, Case, Poisoned, _bits, _bound, _gemm, _lib, _round, _ulp

pytestmark = pytest.mark.gpu

SWITCH = "TCAVT_GEMM_NO_RES_PREFETCH"
MODES = ("s16_res", "s16_res_oop", "s16_res_ns", "s16")


@contextlib.contextmanager
def _prefetch(on):
    """the A/B switch for the calls inside (the library reads it at every launch)"""
    old = os.environ.pop(SWITCH, None)
    if not on:
        os.environ[SWITCH] = "1"
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


class Run:
    """one call of the 16-bit stream form: buffers, status, and what it left behind"""

    def __init__(self, cs, tile, mode, s16, flag_tag=7):
        capi = _lib()
        M, N, dev, dt = cs.M, cs.N, cs.dev, cs.dt
        self.npart = N // 64
        self.ns = 2.0 ** -3 if mode.endswith("_ns") else 1.0
        self.with_res = "res" in mode
        self.H = Poisoned(M, N, dt, dev, fill=s16 if mode != "s16_res_oop" else None)
        self.part = Poisoned(1, M * self.npart, F32, dev, ld=M * self.npart + 64, extra_rows=1)
        self.flag = torch.zeros(4, dtype=torch.int32, device=dev)
        kw = dict(norm_h16=self.H.buf, norm_part=self.part.buf, norm_scale=self.ns if self.ns != 1.0 else 0.0,
                  nonfinite_flag=self.flag, nonfinite_tag=flag_tag, C=None, ldc=self.H.ld)
        self.src = None
        if mode == "s16_res_oop":
            self.src = Poisoned(M, N, dt, dev, ld=self.H.ld, fill=s16)
            kw.update(norm_res16=self.src.buf)
        epi = capi.EPI_NORM_OUT | (capi.EPI_RESIDUAL if self.with_res else 0)
        self.rc = _gemm(**cs.args(tile, out_dtype=capi.F32, epilogue=epi, **kw))

    @property
    def parts(self):
        return self.part.buf[0, : self.H.rows * self.npart].view(self.H.rows, self.npart)


def _check_float64(cs, run, s16, what):
    """the checks of test_norm_out on the 16-bit stream: stream, partial sums, poisoned surroundings, inputs, flag"""
    M, N, dt = cs.M, cs.N, cs.dt
    ref = run.ns * cs.acc + (s16.double() if run.with_res else 0)
    if cs.regime == "exact":
        assert torch.equal(_bits(run.H.region), _bits(_round(ref, dt))), f"{what}: stream"
    else:
        _bound(run.H.region, ref, run.ns * U * cs.abs, 2 * U * ref.abs(), dt, what + " stream")
    if run.src is not None:
        assert torch.equal(_bits(run.src.buf), _bits(run.src.before)), f"{what}: norm_res16 modified"
    run.H.check(what + " h16")
    gw = N // run.npart
    want = run.H.region.double().view(M, run.npart, gw).pow(2).sum(-1)  # partial sums of the ROUNDED values
    assert torch.isfinite(run.parts).all(), f"{what}: partial sums not all written"
    assert ((run.parts.double() - want).abs() <= (gw + 8) * U * want + 1e-30).all(), f"{what}: partial sums"
    run.part.check(what + " part")
    cs.check_inputs()
    assert int(run.flag[0]) == 0, f"{what}: nonfinite flag raised on finite data"


def _check_same(a, b, what):
    """prefetch vs TCAVT_GEMM_NO_RES_PREFETCH=1: whole buffers (poison included) bit for bit"""
    assert torch.equal(_bits(a.H.buf), _bits(b.H.buf)), f"{what}: stream differs from the epilogue with global loads"
    assert torch.equal(_bits(a.part.buf), _bits(b.part.buf)), f"{what}: partial sums differ from the epilogue with global loads"
    assert torch.equal(a.flag, b.flag), f"{what}: nonfinite flag differs"


def _both(cs, tile, mode, s16, what):
    capi = _lib()
    runs = []
    for on in (True, False):
        with _prefetch(on):
            r = Run(cs, tile, mode, s16)
        capi.check(r.rc, what)
        _check_float64(cs, r, s16, f"{what} prefetch={int(on)}")
        runs.append(r)
    _check_same(runs[0], runs[1], what)


def _s16(cs):
    return _round(cs.side((cs.M, cs.N), scale=4.0, den=8).double(), cs.dt)


SHAPES = [(tile, MN, K) for tile in (257, 272) for MN in (256, 512) for K in (64, 128, 192, 256, 320)] + [(272, 512, 4096)]


@pytest.mark.parametrize("regime", ["exact", "real"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_stream_modes(gpu, shape, dt, regime):
    """every K-tile count parity, one and four workgroups, all four stream modes; K = 64 is accepted by both forms (one K-tile)"""
    tile, MN, K = shape
    cs = Case(MN, MN, K, dt, regime, seed=tile * 7 + MN + K, dev=gpu["device"])
    s16 = _s16(cs)
    keep = s16.clone()
    for mode in MODES:
        _both(cs, tile, mode, s16, f"res-prefetch {tile} {mode} {str(dt)[6:]} {regime}: {MN}x{MN}x{K}")
    assert torch.equal(s16, keep)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("tile", [257, 272])
def test_mixed_persistent_launch(gpu, tile, dt):
    """264 tiles on 256 CUs: the launch is persistent, eight workgroups walk two tiles (first: global loads, the look-ahead
    slots carry the next tile's operands; last: prefetch), the other 248 only their last"""
    if gpu["num_cus"] != 256:
        pytest.skip(f"the 248 + 8 split of this test is derived for 256 CUs, this device has {gpu['num_cus']}")
    M, N, K = 8448, 2048, 128
    n_cu = gpu["num_cus"] // 8 * 8  # launch_w4: persistent when tiles > n_cu and K >= 128, one workgroup per CU
    tiles = (M // 256) * (N // 256)
    assert tiles > n_cu and K >= 128 and tiles - n_cu == 8 and tiles < 2 * n_cu
    for regime in ("exact", "real"):
        cs = Case(M, N, K, dt, regime, seed=tile + 3, dev=gpu["device"])
        s16 = _s16(cs)
        for mode in MODES:
            _both(cs, tile, mode, s16, f"res-prefetch persistent {tile} {mode} {str(dt)[6:]} {regime}")


@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("tile,K", [(257, 128), (257, 192), (272, 128), (272, 192)])
def test_inf_residual_raises_flag(gpu, tile, K, dt):
    """one +-inf element of the residual (in either 64-column half of a quadrant, i.e. either LDS buffer) comes out as it went
    in and raises the flag with the call's tag; the rest of the stream is untouched by it"""
    dev = gpu["device"]
    capi = _lib()
    MN = 512
    cs = Case(MN, MN, K, dt, "real", seed=tile + K, dev=dev)
    base = _s16(cs)
    for (m, n), val in (((3, 5), float("inf")), ((300, 70), float("-inf")), ((130, 449), float("inf")), ((511, 300), float("-inf"))):
        s16 = base.clone()
        s16[m, n] = val
        runs = []
        for on in (True, False):
            with _prefetch(on):
                r = Run(cs, tile, "s16_res", s16, flag_tag=11)
            capi.check(r.rc, "inf residual")
            what = f"inf residual {tile} K={K} at {(m, n)} prefetch={int(on)}"
            assert int(r.flag[0]) == 11, f"{what}: flag not raised with the tag"
            got = r.H.region
            assert float(got[m, n]) == val, f"{what}: the element itself"
            mask = torch.ones(MN, MN, dtype=torch.bool, device=dev)
            mask[m, n] = False
            assert torch.isfinite(got[mask]).all(), f"{what}: spread"
            ref = cs.acc + base.double()
            ok = ((got.double() - ref).abs() <= 4.0 * U * cs.abs + 2 * U * ref.abs() + _ulp(ref, dt))[mask]
            assert ok.all(), f"{what}: other elements"
            r.H.check(what)
            runs.append(r)
        _check_same(runs[0], runs[1], f"inf residual {tile} K={K} at {(m, n)}")

