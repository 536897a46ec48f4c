"""CPU emulation of the bf16x3 split arithmetic of the fp32 conv GEMMs (policy key 53; igemm.h).

Every tensor stays fp32; each GEMM operand is split into ``hi = bf16(x)`` and ``lo = bf16(x - hi)``
(round to nearest even) and a conv pass is the sum of three fp32 convs on the split operands,
``hi*hi + (hi*lo + lo*hi)``: the three products the kernels accumulate, without their accumulation
order. Helper of tests/test_bf16x3_host.py and tests/test_gpu_bf16x3*.py (not a test module).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


def split(t: torch.Tensor):
    """fp32 tensor -> (hi, lo) as fp32 tensors holding bf16 values; t - hi is exact in fp32."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def x3(op, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """op(a, b), bilinear in fp32 tensors a and b, on the split operands: hh + (hl + lh)."""
    ah, al = split(a)
    bh, bl = split(b)
    return op(ah, bh) + (op(ah, bl) + op(al, bh))


class ConvX3(torch.autograd.Function):
    """conv2d (no bias, dilation 1, groups 1) whose forward, data gradient and weight gradient are each
    three fp32 convs on split operands."""

    @staticmethod
    def forward(ctx, x, w, stride, padding):
        ctx.save_for_backward(x, w)
        ctx.sp = (stride, padding)
        return x3(lambda a, b: F.conv2d(a, b, stride=stride, padding=padding), x, w)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, padding = ctx.sp
        gy = gy.contiguous()
        gx = x3(lambda g, b: torch.nn.grad.conv2d_input(x.shape, b, g, stride=stride, padding=padding), gy, w)
        gw = x3(lambda a, g: torch.nn.grad.conv2d_weight(a, w.shape, g, stride=stride, padding=padding), x, gy)
        return gx, gw, None, None


def use_x3_convs(model: nn.Module) -> nn.Module:
    """Route every nn.Conv2d of ``model`` (an fp32 oracle model) through ConvX3, in place."""
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            assert m.bias is None and m.groups == 1 and tuple(m.dilation) == (1, 1) and m.weight.dtype == torch.float32
            m.forward = (lambda x, m=m: ConvX3.apply(x, m.weight, tuple(m.stride), tuple(m.padding)))
    return model
