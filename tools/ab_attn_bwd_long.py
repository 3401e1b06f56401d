"""A/B of the attention backward at 256 < T <= 544 (B=32, 32 query / 8 key-value heads, fp16): the chunked two-launch form
(tcavt_attn_bwd_long) against the tiled one-sweep path it replaces (attn_bwd_scores + attn_bwd_dkv + rope_bwd_pack through an
fp32 buffer; TCAVT_ATTN_BWD_NO_LONG).  Both forms alternate in one process, every call timed with HIP events; the median of
the runs after the warm-ups, in us per call, and the ratio.  Usage: python tools/ab_attn_bwd_long.py [T ...]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tcavt_amd import capi, ops
from tcavt_amd.config import LlamaShape
from tcavt_amd.rope import rope_tables

capi.init(0)
dev = torch.device("cuda:0")
B, nq, nkv, dt = 32, 32, 8, torch.float16
RUNS, WARM = 15, 3
Ts = [int(a) for a in sys.argv[1:]] or [320, 384, 512, 528]
print(f"B={B} nq={nq} nkv={nkv} {str(dt)[6:]}; median of {RUNS} runs after {WARM} warm-ups, forms alternating, us per call")
print(f"{'T':>5} {'tiled':>10} {'chunked':>10} {'tiled/chunked':>14}   agreement (rel)")
for T in Ts:
    ncols, M, Tp = (nq + 2 * nkv) * 64, B * T, (T + 63) // 64 * 64
    g = torch.Generator(device="cpu").manual_seed(1)
    qkv = torch.zeros(M + 64, ncols, dtype=dt, device=dev)
    qkv[:M] = torch.randn(M, ncols, generator=g).to(dt).to(dev)
    dO = torch.randn(M, nq * 64, generator=g).to(dt).to(dev)
    kv_len = torch.full((B,), T, dtype=torch.int32, device=dev)
    kv_len[::3] = max(1, T - 37)
    cos, sin = (t.to(dev) for t in rope_tables(LlamaShape(), T))
    att = torch.empty(M, nq * 64, dtype=dt, device=dev)
    lse = torch.empty(B * nq * T, device=dev)
    ops.attn_causal_gqa(qkv[:M], att, kv_len, B, T, nq, nkv, 0.125, lse=lse)
    stats = torch.empty(B * nq * T, 4, device=dev)
    g32 = torch.empty(M, ncols, device=dev)
    out = {"tiled": torch.empty(M, ncols, dtype=dt, device=dev), "chunked": torch.empty(M, ncols, dtype=dt, device=dev)}

    def tiled():
        ops.attn_bwd_scores(qkv, dO, None, None, None, kv_len, B, T, Tp, nq, nkv, 0.125, dQ=g32, stats=stats, lse=lse, att=att)
        ops.attn_bwd_dkv(qkv, dO, stats, g32, kv_len, B, T, Tp, nq, nkv, 0.125)
        ops.rope_bwd_pack(g32, out["tiled"], cos, sin, (nq + nkv) * 64, T)

    def chunked():
        ops.attn_bwd_long(qkv, dO, att, lse, out["chunked"], stats, cos, sin, kv_len, B, T, nq, nkv, 0.125)

    forms = {"tiled": tiled, "chunked": chunked}
    times = {k: [] for k in forms}
    for it in range(WARM + RUNS):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= WARM:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    a, b = statistics.median(times["tiled"]), statistics.median(times["chunked"])
    rel = ((out["chunked"].float() - out["tiled"].float()).norm() / out["tiled"].float().norm()).item()
    print(f"{T:5d} {a:10.1f} {b:10.1f} {a / b:14.2f}   {rel:.2e}", flush=True)
