"""Plain torch twins of the grouped 3x3 convolution (koaf.h "Grouped 3x3 convolution") for the tests: the block-diagonal
64-channel slab images of a grouped weight and the convolution, its data gradient and its weight gradient on NHWC tensors.

Layouts (koaf.h): a packed grouped weight is [C][3][3][Cg], Cg = C / groups input channels per output channel; its slab image is
wexp [C/64][64][9][64] = (slab, output channel of the slab, filter tap, input channel of the slab), zero off the group blocks: output
channel co = 64 z + col reads the slab-local input channels [(col // Cg) * Cg, +Cg).  Every Cg that divides 64 is admitted.

expand / compress only move elements and keep the dtype they are given (they are compared bit for bit); the three convolution
twins compute in `dtype` (float64: the reference; float32: torch's fp32 CPU product of the same operands, for the componentwise
bar of test_tiles_gpu.py).  tests/test_gconv_refs_cpu.py proves them against each other without a GPU."""
import torch
import torch.nn.functional as F


def _cg(C, groups):
    assert C % 64 == 0 and groups > 0 and C % groups == 0 and 64 % (C // groups) == 0, (C, groups)
    return C // groups


def _block_index(C, Cg):
    """[C, Cg] slab-local input channels of every output channel's group block"""
    col = torch.arange(C) % 64
    return ((col // Cg) * Cg)[:, None] + torch.arange(Cg)[None, :]


def expand(w, C, groups):
    """w packed [C,3,3,Cg] (or [C,9,Cg]) -> wexp [C/64, 64, 9, 64], exact zeros off the group blocks"""
    Cg = _cg(C, groups)
    w = w.reshape(C, 9, Cg)
    wexp = torch.zeros(C, 9, 64, dtype=w.dtype, device=w.device)
    idx = _block_index(C, Cg).to(w.device)[:, None, :].expand(C, 9, Cg)
    wexp.scatter_(2, idx, w)
    return wexp.reshape(C // 64, 64, 9, 64)


def compress(dwexp, C, groups):
    """dwexp [C/64, 64, 9, 64] -> dw packed [C,3,3,Cg]: the group blocks, whatever lies off them is ignored"""
    Cg = _cg(C, groups)
    idx = _block_index(C, Cg).to(dwexp.device)[:, None, :].expand(C, 9, Cg)
    return dwexp.reshape(C, 9, 64).gather(2, idx).reshape(C, 3, 3, Cg).contiguous()


def _nchw(t, dtype):
    return t.to(dtype).permute(0, 3, 1, 2)


def gconv64(a, w, stride, groups, dtype=torch.float64):
    """a [N,H,W,C], w packed [C,3,3,Cg] -> y [N,OH,OW,C]: 3x3, pad 1"""
    y = F.conv2d(_nchw(a, dtype), _nchw(w, dtype), stride=stride, padding=1, groups=groups)
    return y.permute(0, 2, 3, 1).contiguous()


def dgrad64(dy, w, shape, stride, groups, dtype=torch.float64):
    """dy [N,OH,OW,C], w packed [C,3,3,Cg], shape = (N, H, W, C) of the input -> dx [N,H,W,C]"""
    N, H, W, C = shape
    dx = torch.nn.grad.conv2d_input((N, C, H, W), _nchw(w, dtype), _nchw(dy, dtype), stride=stride, padding=1, groups=groups)
    return dx.permute(0, 2, 3, 1).contiguous()


def wgrad64(dy, a, stride, groups, dtype=torch.float64):
    """dy [N,OH,OW,C], a [N,H,W,C] -> dw packed [C,3,3,Cg]"""
    C = a.shape[-1]
    dw = torch.nn.grad.conv2d_weight(_nchw(a, dtype), (C, C // groups, 3, 3), _nchw(dy, dtype), stride=stride, padding=1, groups=groups)
    return dw.permute(0, 2, 3, 1).contiguous()


def slab_conv64(a, wexp, stride, dtype=torch.float64):
    """the convolution as the device runs it: one dense 64 -> 64 convolution per slab of wexp over that slab's channels of a"""
    out = []
    for z in range(wexp.shape[0]):
        wz = wexp[z].to(dtype).reshape(64, 3, 3, 64).permute(0, 3, 1, 2)
        yz = F.conv2d(_nchw(a[..., 64 * z:64 * z + 64], dtype), wz, stride=stride, padding=1)
        out.append(yz.permute(0, 2, 3, 1))
    return torch.cat(out, dim=-1).contiguous()
