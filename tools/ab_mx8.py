"""A/B of the opt-in MX8 MLP against the 16-bit kernels, one process, one device, the arms alternating.  Measurement only.

1. per launch, at the Llama-3.2-1B decoder's shapes (M = 8192 = 32 x 256 rows, fp16, the stage's flag sets): gate|up (N = 16384,
   K = 2048, SILU_MUL | ROWSCALE) and down (N = 2048, K = 8192, RESIDUAL | NORM_OUT on the in-place 16-bit stream) as
   tcavt_gemm_bf16 (tile 0: what the decoder runs), as tcavt_gemm_mx8 alone (operands already quantised) and as
   tcavt_quant_mx8 + tcavt_gemm_mx8 (what an MX8 layer launches).  The activation operand is re-written by a copy kernel before
   every launch, 8 rotating weight matrices; every launch (pair) has its own event pair.
2. the model forward (eval, loss + decoded) at config 2's shape (B = 32, L = 256) and at config 5's (T_in 6, T_out 12, L = 256,
   B = 512 unless given), set_mlp_precision("fp16") and ("mx8") alternating.

usage: ab_mx8.py [rounds per arm, default 30] [config-5 batch, default 512]
"""
import ctypes
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tcavt_amd import capi, config, model, ops, synth  # noqa: E402
from tcavt_amd.weights import make_weights  # noqa: E402


def _stats(name, ts):
    ts = sorted(ts)
    k = len(ts)
    print(f"  {name:18s}: median {ts[k // 2]:8.2f}  min {ts[0]:8.2f}  max {ts[-1]:8.2f}  quartiles {ts[k // 4]:8.2f} / {ts[3 * k // 4]:8.2f}"
          f"  ({k} runs)", flush=True)
    return ts[k // 2]


def kernels(rounds, dev):
    dt, M, H, I = torch.float16, 8192, 2048, 8192
    for name, (N, K) in (("gate|up", (2 * I, H)), ("down", (H, I))):
        a_src = (torch.randn(M, K, device=dev) * (1.0 if name == "gate|up" else 0.2)).to(dt)
        a = a_src.clone()
        ws = [(torch.randn(N, K, device=dev) / math.sqrt(K)).to(dt) for _ in range(8)]
        w8 = [ops.quant_mx8(w) for w in ws]
        a8 = ops.quant_mx8(a)
        part = torch.rand(M, H // 64, device=dev) * 64 + 1
        h16 = torch.randn(M, H, device=dev).to(dt)
        act = torch.empty(M, I, dtype=dt, device=dev)
        silu = name == "gate|up"

        def fp16(i):
            g = capi.GemmArgs()
            g.A, g.lda, g.W, g.ldw = a.data_ptr(), K, ws[i % 8].data_ptr(), K
            g.M, g.N, g.K, g.in_dtype = M, N, K, capi.F16
            if silu:
                g.C, g.ldc, g.out_dtype, g.epilogue = act.data_ptr(), I, capi.F16, capi.EPI_SILU_MUL | capi.EPI_ROWSCALE
                g.rowscale_part, g.rowscale_npart, g.rowscale_h, g.rowscale_eps = part.data_ptr(), H // 64, H, 1e-5
            else:
                g.C, g.ldc, g.out_dtype, g.epilogue = None, H, capi.F32, capi.EPI_RESIDUAL | capi.EPI_NORM_OUT
                g.norm_h16, g.norm_part = h16.data_ptr(), part.data_ptr()
            capi.check(capi.lib().tcavt_gemm_bf16(ctypes.byref(g), capi.stream_ptr()), "gemm_bf16")

        def mx8(i, quantise):
            if quantise:
                ops.quant_mx8(a, *a8)
            if silu:
                ops.gemm_mx8(a8[0], a8[1], w8[i % 8][0], w8[i % 8][1], act, dt, epilogue=capi.EPI_SILU_MUL | capi.EPI_ROWSCALE,
                             rowscale_part=part, rowscale_npart=H // 64, rowscale_h=H, rowscale_eps=1e-5)
            else:
                ops.gemm_mx8(a8[0], a8[1], w8[i % 8][0], w8[i % 8][1], None, dt, epilogue=capi.EPI_RESIDUAL | capi.EPI_NORM_OUT,
                             ldc=H, norm_h16=h16, norm_part=part)

        arms = ("fp16 gemm", "mx8 gemm", "mx8 quant + gemm")
        n = 3 * rounds
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        arm_of = []
        for i in range(n + 9):
            arm = (i + i // 3) % 3  # the order rotates from round to round
            a.copy_(a_src)
            if not silu:
                h16.normal_()  # (the in-place stream would random-walk out of range over the launches)
            if i >= 9:
                ev[i - 9][0].record()
            if arm == 0:
                fp16(i)
            else:
                mx8(i, arm == 2)
            if i >= 9:
                ev[i - 9][1].record()
                arm_of.append(arm)
        torch.cuda.synchronize()
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        print(f"{name}  M x N x K = {M} x {N} x {K}, us per launch", flush=True)
        med = [_stats(nm, [t for t, k in zip(us, arm_of) if k == j]) for j, nm in enumerate(arms)]
        flop = 2.0 * M * N * K
        print(f"  PFLOP/s at the medians: fp16 {flop / med[0] * 1e-9:.3f}, mx8 gemm {flop / med[1] * 1e-9:.3f}, mx8 quant + gemm "
              f"{flop / med[2] * 1e-9:.3f};  mx8 quant + gemm / fp16 = {med[2] / med[0]:.3f}", flush=True)


def forward(label, cfg, B, rounds, dev):
    with torch.device(dev):
        m = model.MultiModalTrajectoryModel.from_config(cfg)
    m.load_weights(make_weights(cfg, seed=1, backend="torch", device=dev)).eval()
    b = synth.make_batch(cfg, B, text_len=240, seed=3, ragged=True, min_text=128)
    g = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}

    def fwd():
        return m(g["traj_emb"], g["vision_emb"], None, g["lane_polygon"], g["lane_polygon_len"], input_ids=g["input_ids"],
                 attention_mask=g["attention_mask"], labels=g["labels"], y=g["target_traj"], norm_stat=g["norm_stat"])

    out = {}
    with torch.no_grad():
        for prec in ("fp16", "mx8", "fp16", "mx8"):  # warm-up: packed weights, MX8 images, workspaces
            m.set_mlp_precision(prec)
            out[prec] = fwd()
        torch.cuda.synchronize()
        m.mllm.check_flags()
        ts = {"fp16": [], "mx8": []}
        for i in range(2 * rounds):
            prec = ("fp16", "mx8")[(i + i // 2) % 2]
            m.set_mlp_precision(prec)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fwd()
            e1.record()
            torch.cuda.synchronize()
            ts[prec].append(e0.elapsed_time(e1))
    m.mllm.check_flags()
    print(f"{label}: model forward, B = {B}, ms", flush=True)
    med = {p: _stats(p, t) for p, t in ts.items()}
    d16, d8 = out["fp16"][1].double(), out["mx8"][1].double()
    print(f"  mx8 / fp16 = {med['mx8'] / med['fp16']:.3f};  decoded mx8 vs fp16: relative L2 {((d8 - d16).norm() / d16.norm()).item():.3e};  "
          f"loss fp16 {out['fp16'][0].item():.4f}  mx8 {out['mx8'][0].item():.4f}", flush=True)
    del m
    torch.cuda.empty_cache()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    b5 = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    capi.init(0)
    dev = torch.device("cuda:0")
    kernels(rounds, dev)
    forward("config 2 (T_in 18, T_out 30, L = 256)", config.PRESETS["llama32_1b"](), 32, max(4, rounds // 3), dev)
    forward("config 5 (T_in 6, T_out 12, L = 256)", config.PRESETS["llama32_1b"](seq_len=6, out_len=12, use_lora=True), b5, max(3, rounds // 10), dev)


if __name__ == "__main__":
    main()
