"""Weight re-layouts the kernels expect (done once at model load, on the host or GPU)."""
import torch

XATTN_PAD = 64  # key counts of the head cross-attention are padded to a multiple of this
# Packed LoRA layout: a_cat [64, H] holds A_q in rows [0, r) and A_v in rows [LORA_V, LORA_V + r); b_ext [nqkv, 64] holds B_q in
# columns [0, r) of the q rows and B_v in columns [LORA_V, LORA_V + r) of the v rows; everything else is zero.  The two adapters
# sit in separate 16-column groups so that, with LoRA dropout on, each down-projection can be a GEMM of its own (N = 16) on its
# own dropped input -- PEFT gives every adapted Linear its own lora_dropout module (independent masks for q_proj and v_proj).
LORA_V = 16

def interleave_gate_up(w_gate, w_up):
    """[I,K] gate and [I,K] up -> [2I,K] with rows interleaved in blocks of 16:
    rows 32j..32j+15 = gate features 16j..16j+15, rows 32j+16..32j+31 = up features 16j..16j+15
    (layout required by TCAVT_EPI_SILU_MUL, include/tcavt.h)."""
    I, K = w_gate.shape
    assert w_up.shape == (I, K) and I % 16 == 0
    g = w_gate.reshape(I // 16, 16, K)
    u = w_up.reshape(I // 16, 16, K)
    return torch.stack([g, u], dim=1).reshape(2 * I, K).contiguous()
