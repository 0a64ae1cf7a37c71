"""Weight gradients of the BEV tail's stock convolutions in a fixed summation order.

MIOpen's backward-weights solvers for the convolutions that do not run on libspx kernels (the stride-2 3x3 down-sampling
conv, the kernel = stride transposed up-sampling convs, the 1x1 head) split their reduction over the pixels in an order
that changes from run to run, so two identical training steps differ in the last bits — and AdamW's first steps
(~lr * sign(grad)) turn that into visibly different weights.  Its deterministic solvers are the naive reference kernels
(~26x slower step).  Here the reduction is a GEMM over pixel rows cut into fixed chunks: one batched GEMM of the chunks,
then a sum over chunks — same fp32 dot products, same order every run.  The data gradient stays MIOpen's (deterministic).
Measurements: profiles/bev_wgrad_determinism.md; tests/test_gpu_bench.py::test_bench_outputs_repeat_bit_for_bit.
"""
import torch
import torch.nn.functional as F

CHUNK = 4096        # pixel rows per partial product


def mm_fixed(at, b):
    """at [M, K] @ b [K, N] (any strides) with K reduced in a fixed order: K cut into chunks of CHUNK, one batched GEMM of
    the chunk products, their sum in chunk order, then the remainder."""
    k = at.shape[1]
    s = k // CHUNK
    if s <= 1:
        return at @ b
    kk = s * CHUNK
    parts = torch.bmm(at[:, :kk].unflatten(1, (s, CHUNK)).transpose(0, 1), b[:kk].unflatten(0, (s, CHUNK)))
    out = parts.sum(0)
    if kk < k:
        out = out + at[:, kk:] @ b[kk:]
    return out


def rows_tn(a, b):
    """a [K, M], b [K, N] -> a^T @ b [M, N], K reduced in a fixed order."""
    return mm_fixed(a.t(), b)


def _rows(t):
    """[N, C, H, W] -> [N*H*W, C] (a view for channels_last maps)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, padding, transposed):
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, padding, transposed)
        if transposed:
            return F.conv_transpose2d(x, w, None, stride)
        return F.conv2d(x, w, None, stride, padding)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, padding, transposed = ctx.cfg
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.ops.aten.convolution_backward(dy, x, w, None, [stride] * 2, [padding] * 2, [1, 1], transposed,
                                                     [0, 0], 1, [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            n = x.shape[0]
            if transposed:                     # kernel == stride: every output pixel has exactly one input pixel
                s, co = stride, w.shape[1]
                h, wd = x.shape[2], x.shape[3]
                d = dy.permute(0, 2, 3, 1).reshape(n, h, s, wd, s, co).permute(0, 1, 3, 5, 2, 4).reshape(n * h * wd, co * s * s)
                dw = rows_tn(_rows(x), d).view_as(w)
            else:
                # one sample at a time (its im2col [Ci*k*k, L] is the GEMM's left operand as unfold writes it), samples
                # summed in order
                k, co = w.shape[2], w.shape[0]
                acc = None
                for i in range(n):
                    cols = F.unfold(x[i:i + 1], k, padding=padding, stride=stride)[0]          # [Ci*k*k, L]
                    part = mm_fixed(cols, dy[i].permute(1, 2, 0).reshape(-1, co))             # [Ci*k*k, Co]
                    acc = part if acc is None else acc + part
                dw = acc.t().reshape(w.shape)
        return dx, dw, None, None, None


def usable(x, m):
    """True when `m` (no bias, square, dilation 1, groups 1; transposed only with kernel == stride) can go through here:
    fp32 CUDA map in training."""
    if not (x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled() and m.weight.requires_grad
            and m.bias is None and m.groups == 1 and tuple(m.dilation) == (1, 1) and not torch.is_autocast_enabled()):
        return False
    k, s = tuple(m.kernel_size), tuple(m.stride)
    if k[0] != k[1] or s[0] != s[1]:
        return False
    if isinstance(m, torch.nn.ConvTranspose2d):
        return k == s and tuple(m.padding) == (0, 0) and tuple(m.output_padding) == (0, 0)
    return isinstance(m, torch.nn.Conv2d)


def conv2d(x, m, padding):
    """m(x) for a Conv2d with `padding` (symmetric) in place of its own."""
    return _ConvFn.apply(x, m.weight, int(m.stride[0]), int(padding), False)


def conv_transpose2d(x, m):
    return _ConvFn.apply(x, m.weight, int(m.stride[0]), 0, True)


def pointwise_wgrad(dy_rows, x_rows):
    """Weight and bias gradient of a 1x1 conv from pixel rows dy [P, Co], x [P, Ci]: [Co, Ci], [Co]."""
    return rows_tn(dy_rows, x_rows), dy_rows.sum(0)
