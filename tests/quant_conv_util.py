"""Shared builders for the int8 convolution tests (CPU and GPU files)."""
import torch

from cloudtik_amd import ops
from cloudtik_amd.models.resnet import ResNet


def randomize_bn(module, g):
    """Every BatchNorm gets a random weight in [0.5, 1.5], bias, running mean and a variance in
    [0.5, 2]: the default zero_init of bn3 would fold conv3 to all-zero weights."""
    for m in module.modules():
        if hasattr(m, "running_var"):
            c = m.weight.shape[0]
            with torch.no_grad():
                m.weight.copy_(torch.rand(c, generator=g) + 0.5)
                m.bias.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
    return module


def tiny_resnet(seed=0, num_classes=10, dtype=torch.float32):
    """resnet_tiny (one bottleneck per stage) on the CPU with random BatchNorm parameters."""
    torch.manual_seed(seed)
    m = ResNet((1, 1, 1, 1), num_classes, dtype=torch.float32)
    randomize_bn(m, torch.Generator().manual_seed(seed + 1))
    return m.to(dtype).eval()


def tiny_images(n=8, size=32, seed=2):
    return torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(seed))


def conv_case(N, H, W, ci, co, R, seed):
    """Random operands of one convolution: int8 image (channels_last), quantized tap-major weight
    rows with their scales, fp32 bias."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-127, 128, (N, ci, H, W), generator=g, dtype=torch.int8).contiguous(
        memory_format=torch.channels_last)
    w = torch.randn(co, R * R * ci, generator=g) * (R * R * ci) ** -0.5
    w_q, w_s = ops.quantize_weight(w)
    bias = torch.randn(co, generator=g) * 0.3
    return x, w_q, w_s, bias


def shifted(x, r, s, R, stride):
    """What a one-hot filter at tap (r, s) of an R x R convolution with padding R // 2 gives:
    the input shifted by the tap, zero beyond the border, sampled at ``stride``."""
    p = R // 2
    N, C, H, W = x.shape
    xp = torch.zeros(N, C, H + 2 * p, W + 2 * p, dtype=x.dtype)
    xp[:, :, p:p + H, p:p + W] = x
    Ho, Wo = (H + 2 * p - R) // stride + 1, (W + 2 * p - R) // stride + 1
    return xp[:, :, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride]


def one_hot_rows(ci, R, r, s):
    """int8 weight rows [ci, R*R*ci] with a 1 at (tap (r, s), channel c) of row c."""
    w = torch.zeros(ci, R * R * ci, dtype=torch.int8)
    idx = torch.arange(ci)
    w[idx, (r * R + s) * ci + idx] = 1
    return w
