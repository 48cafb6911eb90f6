"""Host-only references of the AST / ViT encoder's dropout kernels (csrc/tf_dropout.hip and the DROP instantiations of
csrc/attention.hip / csrc/attention_sp.hip), and the case lists of tests/test_encoder_dropout_kernels_gpu.py
(tests/test_encoder_dropout_kernels_cpu.py asserts from the sources that they reach every dispatch branch).

hash_keep restates the generator of csrc/eav_common.h (eav_hash32 / dropout_keep) in numpy uint64 arithmetic; the
attention and softmax references are plain float64 torch under an explicit keep-mask."""
import numpy as np
import torch

M64 = (1 << 64) - 1
HD = 64                                            # head_dim of the fused kernels

# ---- case lists (B, H, N) ---------------------------------------------------------------------------------------------
# fused fp32 kernels: one ragged key tile (N <= 32), exact multiples of 32 / 128 (no ragged tile), either side of the
# 128-row workgroup, more than 4 image-heads, the reduced models' 197 / 302 tokens and the workload's 1214
ATTN_CASES = [(1, 1, 1), (1, 1, 31), (1, 1, 32), (1, 1, 33), (2, 2, 64), (2, 3, 70), (3, 3, 128), (3, 4, 129), (2, 3, 197),
              (1, 2, 302), (1, 2, 1214)]
ATTN_P = [0.1, 0.5, 0.9]
# split kernels: 9 / 12 / 16 image-heads = full groups of 8 on the XCD-aware workgroup map with and without a remainder;
# N = 128 / 129: either side of the 2-wave / 4-wave forward
SP_CASES = [(1, 1, 31), (1, 2, 64), (4, 4, 70), (3, 3, 128), (3, 4, 129), (2, 3, 197), (2, 2, 302), (1, 2, 1214)]
SP_P = [0.1, 0.5, 0.51, 0.75, 0.9]                 # 2^e >= 1 / (1 - p): e = 1, 1, 2, 2, 4
SP_DO = [1e-3, 1.0]
SP_SPIKE = (2, 2, 302, 3.0)                        # (B, H, N, std of qkv) of the one spike case
SOFTMAX_N = [1, 63, 64, 65, 256, 257, 1280, 1281, 2048]
SOFTMAX_ROWS = [5, 8]                              # four rows per block: 5 leaves a partial block
SOFTMAX_P = [0.1, 0.9]
EW_CAP = 8192 * 256                                # elements one pass of the element-wise grids covers
MASK_N = [1, 255, 4096, EW_CAP + 1]
ADD_N = [4, 1028, 4 * EW_CAP + 20]                 # float4 elements: n / 4
GEN_P = [0.1, 0.5, 0.9]


def hash_keep(seed, n, p, counter=None):
    """dropout_keep(p, seed', idx) for idx = 0 .. n-1 without a mask, seed' = seed + 2 counter (mod 2^64): uint8 [n]."""
    seed = (int(seed) + (0 if counter is None else 2 * int(counter))) & M64
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    h = (z >> np.uint64(40)).astype(np.float32)    # 24 bits: exact in fp32, and so is the product with 2^-24
    return (h * np.float32(2.0 ** -24) >= np.float32(p)).astype(np.uint8)


def scale32(p):
    """The kernels' dropout_scale: 1 / (1 - p) in fp32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def sp_exponent(p):
    """make_sp_drop's e (csrc/attention_sp.hip): the smallest e with 2^e >= fp32(1 / (1 - p))."""
    iq, e = np.float32(scale32(p)), 0
    while np.float32(1 << e) < iq and e < 30:
        e += 1
    return e


def planted_mask(seed, B, H, N, p):
    """hash_keep mask [B, H, N, N] with planted rows and columns (N > 1).  Image-head 0: query row 1 kept, key column 2
    dropped (in every row: the dropped column wins over the kept row at element (1, 2), so that dV of key 2 is exactly 0),
    query row 0 dropped; last image-head: the last query row dropped."""
    m = hash_keep(seed, B * H * N * N, p).reshape(B, H, N, N).copy()
    if N > 1:
        m[0, 0, 1, :] = 1
        m[0, 0, :, 2] = 0
        m[0, 0, 0, :] = 0
        m[-1, -1, -1, :] = 0
    return m


def attention_ref(qkv, dO, mask, B, H, N, p, dtype=torch.float64):
    """qkv [B*N, 3D] (Q | K | V, head h at columns 64 h), dO [B*N, D], keep-mask [B, H, N, N] -> O [B*N, D],
    dqkv [B*N, 3D] (autograd), lse [B*H, N] of the UNDROPPED scaled scores.  O = (P o M scale32(p)) V."""
    D = H * HD
    x = torch.as_tensor(qkv).to(dtype).view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    s = (x[0] @ x[1].transpose(-1, -2)) * HD ** -0.5
    pd = torch.softmax(s, -1) * (torch.as_tensor(mask).to(dtype).view(B, H, N, N) * scale32(p))
    out = (pd @ x[2]).permute(0, 2, 1, 3).reshape(B * N, D)
    out.backward(torch.as_tensor(dO).to(dtype))
    return (out.detach(), x.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * D),
            torch.logsumexp(s, -1).reshape(B * H, N).detach())


def softmax_dropout_ref(scores, dP, mask, p, P=None):
    """scores, dP, mask [rows, N] -> float64 P = softmax(scores), Pd = P o M s, dS = P o (M o dP s - rowsum(P o M o dP s))
    with s = scale32(p), and the magnitude |P| (|M o dP s| + sum |P o M o dP s|) the bound of dS is stated in.
    P (optional): the probabilities the backward is given (the kernel's own fp32 P) instead of softmax(scores)."""
    Pr = torch.softmax(torch.as_tensor(scores).double(), -1)
    Pb = Pr if P is None else torch.as_tensor(P).double()
    g = torch.as_tensor(mask).double() * torch.as_tensor(dP).double() * scale32(p)
    dS = Pb * (g - (Pb * g).sum(-1, keepdim=True))
    mag = Pb.abs() * (g.abs() + (Pb * g).abs().sum(-1, keepdim=True))
    return Pr, Pr * torch.as_tensor(mask).double() * scale32(p), dS, mag
