"""A/B of the residual prefetch of the o / down projections (csrc/gemm_w4.hpp), one process, one device.  Measurement only.

The in-model calls (M = 8192, N = 2048, K = 2048 / 8192, fp16, in-place 16-bit stream with residual, tile 0), operands as in the
"fresh" leg of tools/insitu_probe.py: the activation operand is re-written by a copy kernel right before every launch, 16
rotating weight matrices.  TCAVT_GEMM_NO_RES_PREFETCH is toggled from launch to launch (the library reads it at every launch), each
launch timed by its own event pair.  Prints median, minimum, maximum and the quartiles of each arm; the prefetch counts as a gain
for a kernel only if its median is below the MINIMUM of the arm with the switch set.  A third arm runs the same launch WITHOUT
the residual flag (nothing is read for the epilogue, a pure store stream behind the same main loop): prefetch minus that arm
bounds everything the prefetch still costs, a slow-down of the last K-tiles by the DMA in flight included.

usage: ab_res_prefetch.py [rounds per arm, default 40]
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tcavt_amd import capi  # noqa: E402

SWITCH = "TCAVT_GEMM_NO_RES_PREFETCH"


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    capi.init(0)
    dev = torch.device("cuda:0")
    dt = torch.float16
    for shape, (M, N, K) in (("o", (8192, 2048, 2048)), ("down", (8192, 2048, 8192))):
        a = (torch.randn(M, K, device=dev) * 0.2).to(dt)
        a_src = a.clone()
        ws = [(torch.randn(N, K, device=dev) * 0.02).to(dt) for _ in range(16)]
        h16 = torch.randn(M, N, device=dev).to(dt)
        pout = torch.empty(M, N // 64, device=dev)

        def launch(w, residual=True):
            g = capi.GemmArgs()
            g.A, g.lda, g.W, g.ldw = a.data_ptr(), K, w.data_ptr(), K
            g.M, g.N, g.K, g.tile = M, N, K, 0
            g.in_dtype = capi.F16
            g.C, g.ldc, g.out_dtype = None, N, capi.F32
            g.epilogue = (capi.EPI_RESIDUAL if residual else 0) | capi.EPI_NORM_OUT
            g.norm_h16, g.norm_part = h16.data_ptr(), pout.data_ptr()
            capi.check(capi.lib().tcavt_gemm_bf16(ctypes.byref(g), capi.stream_ptr()), "gemm")

        n = 3 * rounds
        arm_of = []
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for i in range(n + 9):
            arm = (i + i // 3) % 3  # the order rotates from round to round: no arm always follows the same one
            if arm == 1:  # arm 1: the switch set (global loads in the epilogue); arm 2: no residual at all
                os.environ[SWITCH] = "1"
            else:
                os.environ.pop(SWITCH, None)
            a.copy_(a_src)
            if i >= 9:
                ev[i - 9][0].record()
            launch(ws[i % 16], residual=arm != 2)
            if i >= 9:
                ev[i - 9][1].record()
            if i >= 9:
                arm_of.append(arm)
        os.environ.pop(SWITCH, None)
        torch.cuda.synchronize()
        assert torch.isfinite(h16).all()
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
        arms = {name: sorted(t for t, k in zip(us, arm_of) if k == j) for j, name in enumerate(("prefetch", "switch set", "no residual"))}
        for name, ts in arms.items():
            k = len(ts)
            print(f"{shape:5s} {M}x{N}x{K} {name:11s}: median {ts[k // 2]:7.2f} us  min {ts[0]:7.2f}  max {ts[-1]:7.2f}  "
                  f"quartiles {ts[k // 4]:7.2f} / {ts[3 * k // 4]:7.2f}  ({k} launches)", flush=True)
        p, s, z = arms["prefetch"], arms["switch set"], arms["no residual"]
        print(f"{shape:5s} prefetch median - switch-set minimum = {p[len(p) // 2] - s[0]:+.2f} us;  median - median = "
              f"{p[len(p) // 2] - s[len(s) // 2]:+.2f} us;  prefetch median - no-residual median = "
              f"{p[len(p) // 2] - z[len(z) // 2]:+.2f} us", flush=True)


if __name__ == "__main__":
    main()
