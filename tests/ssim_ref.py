"""Restatements of the SSIM contract in include/voxe.h (voxe_ssim_fwd_bwd) and the fixtures its tests share.

Images are channel-last [N,H,W,C] torch tensors.  Wang et al. 2004: an 11 x 11 Gaussian window of sigma 1.5 (normalised in double,
rounded to float), VALID windows only, C1 = (0.01 L)^2, C2 = (0.03 L)^2.
  ssim64          float64, S by direct 2-D windows; the gradient to x comes from float64 autograd (ssim64_grad)
  closed_form64   the P / Q / R maps and the gradient formula of the contract, float64
  ssim32_torch    a float32 restatement the way one would write it in torch (separable grouped conv2d + autograd): the yardstick
                  whose own error against ssim64 bounds the kernel's
  `pad`, `sigma`, `drop_q` restate it WRONGLY on purpose: the host test shows the GPU test's bounds tell them apart."""
import os

import numpy as np
import torch
import torch.nn.functional as F

WIN = 11
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gaussian(sigma: float = 1.5, rounded: bool = True) -> torch.Tensor:
    """the 1-D window: normalised to sum 1 in double, then rounded to float (returned as float64 of those floats); rounded=False
    keeps the double window other packages use"""
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2) / (2.0 * sigma * sigma))
    g = g / g.sum()
    return torch.from_numpy(g.astype(np.float32).astype(np.float64) if rounded else g)


def constants(data_range: float = 1.0):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def _moments(x: torch.Tensor, y: torch.Tensor, sigma: float, pad: bool, rounded: bool = True):
    """the five window sums by direct 2-D windows: [N,Ho,Wo,C] each"""
    g = gaussian(sigma, rounded).to(x.dtype)
    g2 = torch.outer(g, g)
    if pad:   # WRONG on purpose: zero-padded ("same") windows
        x, y = (F.pad(t, (0, 0, WIN // 2, WIN // 2, WIN // 2, WIN // 2)) for t in (x, y))

    def win(t):
        return (t.unfold(1, WIN, 1).unfold(2, WIN, 1) * g2).sum(dim=(-2, -1))   # [N,Ho,Wo,C,11,11] -> [N,Ho,Wo,C]

    return win(x), win(y), win(x * x), win(y * y), win(x * y)


def _terms(mx, my, mxx, myy, mxy, data_range):
    C1, C2 = constants(data_range)
    vx, vy, vxy = mxx - mx * mx, myy - my * my, mxy - mx * my
    return 2 * mx * my + C1, 2 * vxy + C2, mx * mx + my * my + C1, vx + vy + C2


def ssim64(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, sigma: float = 1.5, pad: bool = False,
           rounded_window: bool = True):
    """(mean, per_image [N], map [N,H-10,W-10,C]) in the dtype of x (float64 in the tests); differentiable"""
    A1, A2, B1, B2 = _terms(*_moments(x, y, sigma, pad, rounded_window), data_range)
    S = A1 * A2 / (B1 * B2)
    return S.mean(), S.mean(dim=(1, 2, 3)), S


def ssim64_grad(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, **kw) -> torch.Tensor:
    """d mean / d x by autograd, float64"""
    xg = x.detach().double().clone().requires_grad_(True)
    ssim64(xg, y.detach().double(), data_range, **kw)[0].backward()
    return xg.grad


def closed_form64(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, drop_q: bool = False):
    """(P, Q, R [N,Ho,Wo,C], gradient [N,H,W,C]) by the formulas of the contract; `drop_q` (WRONG on purpose) leaves the Q term out"""
    x, y = x.double(), y.double()
    mx, my, mxx, myy, mxy = _moments(x, y, 1.5, False)
    A1, A2, B1, B2 = _terms(mx, my, mxx, myy, mxy, data_range)
    S = A1 * A2 / (B1 * B2)
    Q = -S / B2
    R = 2 * A1 / (B1 * B2)
    P = 2 * my * (A2 - A1) / (B1 * B2) + 2 * mx * S * (1 / B2 - 1 / B1)
    g = gaussian()
    C = x.shape[-1]
    w = torch.outer(g, g)[None, None].repeat(C, 1, 1, 1)

    def full(m):   # the transpose of the valid correlation: sum over the windows q that contain p of g(p - q) m_q
        return F.conv_transpose2d(m.permute(0, 3, 1, 2), w, groups=C).permute(0, 2, 3, 1)

    grad = full(P) + y * full(R)
    if not drop_q:
        grad = grad + 2 * x * full(Q)
    return P, Q, R, grad / S.numel()


def ssim32_torch(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0):
    """float32, separable grouped conv2d, the textbook variance form; (mean, per_image, map), differentiable w.r.t. x.  Runs on
    the device of x."""
    x, y = x.float(), y.float()
    C = x.shape[-1]
    g = gaussian().to(device=x.device, dtype=torch.float32)
    wh, wv = g.view(1, 1, 1, WIN).repeat(C, 1, 1, 1), g.view(1, 1, WIN, 1).repeat(C, 1, 1, 1)

    def blur(t):
        return F.conv2d(F.conv2d(t, wh, groups=C), wv, groups=C)

    xc, yc = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    mx, my = blur(xc), blur(yc)
    A1, A2, B1, B2 = _terms(mx, my, blur(xc * xc), blur(yc * yc), blur(xc * yc), data_range)
    S = (A1 * A2 / (B1 * B2)).permute(0, 2, 3, 1)
    return S.mean(), S.mean(dim=(1, 2, 3)), S


def ssim32_torch_grad(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    xg = x.detach().float().clone().requires_grad_(True)
    ssim32_torch(xg, y.detach(), data_range)[0].backward()
    return xg.grad


# ---- fixtures: (x, y) float32 [N,H,W,C] in [0, 1], on the CPU ------------------------------------------------------------
def _blur3(t: torch.Tensor) -> torch.Tensor:
    C = t.shape[-1]
    k = torch.full((C, 1, 3, 3), 1.0 / 9.0, dtype=t.dtype)
    return F.conv2d(F.pad(t.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate"), k, groups=C).permute(0, 2, 3, 1)


def noise(seed: int, N: int, H: int, W: int, C: int):
    """uniform noise in [0, 1] (the target) and a blurred + perturbed copy of it"""
    gen = torch.Generator().manual_seed(seed)
    y = torch.rand((N, H, W, C), generator=gen)
    x = (0.6 * y + 0.4 * _blur3(y) + 0.05 * torch.randn((N, H, W, C), generator=gen)).clamp(0.0, 1.0)
    return x.contiguous(), y.contiguous()


def white_background(N: int, H: int, W: int, C: int, seed: int = 7):
    """a textured disc on an exact 1.0 surround in BOTH images; the disc sits in a corner and is small enough that at least half
    of the windows see only the surround (white_only_windows says which)"""
    gen = torch.Generator().manual_seed(seed)
    rows, cols = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    radius = max(2.5, 0.2 * min(H, W))
    disc = ((rows - radius) ** 2 + (cols - radius) ** 2 <= radius * radius)[None, :, :, None]
    y = torch.where(disc, 0.15 + 0.7 * torch.rand((N, H, W, C), generator=gen), torch.ones(()))
    x = torch.where(disc, (0.3 * y + 0.6 * torch.rand((N, H, W, C), generator=gen)).clamp(0.0, 1.0), torch.ones(()))
    return x.contiguous(), y.contiguous()


def white_only_pixels(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] bool: pixels all of whose windows see only the exact-1.0 surround in both images (their gradient is exactly 0)"""
    flat = ((x == 1.0) & (y == 1.0)).all(dim=-1, keepdim=True).float().permute(0, 3, 1, 2)
    windows = -F.max_pool2d(-flat, WIN, stride=1)                                    # 1 where a window is all surround
    dirty = F.max_pool2d(F.pad(1.0 - windows, (WIN - 1,) * 4), WIN, stride=1)      # 1 where a pixel lies in a window that is not
    return (dirty == 0).permute(0, 2, 3, 1).expand_as(x)


def white_only_windows(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    flat = ((x == 1.0) & (y == 1.0)).all(dim=-1, keepdim=True).float().permute(0, 3, 1, 2)
    return (-F.max_pool2d(-flat, WIN, stride=1) == 1).permute(0, 2, 3, 1)


def rendered(N: int, H: int, W: int, C: int, seed: int = 3):
    """crops of the golden renders (tests/golden/frames32.npz, 8 frames of 64 x 64 x 3) as targets, a softened + perturbed copy
    as the image; a 4th channel is the mean of the three"""
    frames = torch.from_numpy(np.load(os.path.join(GOLDEN, "frames32.npz"))["frames"])
    assert N <= frames.shape[0] and H <= frames.shape[1] and W <= frames.shape[2]
    top, left = (frames.shape[1] - H) // 2, (frames.shape[2] - W) // 2
    y = frames[:N, top:top + H, left:left + W, :]
    if C == 4:
        y = torch.cat([y, y.mean(dim=-1, keepdim=True)], dim=-1)
    y = y[..., :C].contiguous()
    gen = torch.Generator().manual_seed(seed)
    x = (0.5 * y + 0.5 * _blur3(y) + 0.02 * torch.randn(y.shape, generator=gen)).clamp(0.0, 1.0)
    return x.contiguous(), y


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---- the cases and bounds of tests/test_ssim_gpu.py (shared with the host test's teeth) ----------------------------------
# (fixture, N, H, W, C): 11 x 11 is one window, 12 x 27 ragged on both axes, 26 x 26 exactly one tile of windows, 27 x 43 one
# tile + 1 and two tiles + 1, 48 x 40 several tiles; every N in {1, 3} and C in {1, 3, 4}; the ragged shapes with every C
CASES = [
    ("noise", 1, 11, 11, 1), ("rendered", 3, 11, 11, 3),
    ("rendered", 1, 12, 27, 1), ("noise", 3, 12, 27, 3), ("noise", 1, 12, 27, 4),
    ("white_background", 1, 26, 26, 3),
    ("white_background", 3, 27, 43, 1), ("noise", 1, 27, 43, 3), ("rendered", 1, 27, 43, 4),
    ("white_background", 3, 48, 40, 3), ("noise", 1, 48, 40, 4),
]
_references = {}


def make(case):
    name, N, H, W, C = case
    if name == "noise":
        return noise(100 + H + C, N, H, W, C)
    return {"white_background": white_background, "rendered": rendered}[name](N, H, W, C)


def reference(case):
    """float64 values and gradient of a case, and the bounds the kernel has to meet on it (computed once, never changed).
    Yardstick: the float32 torch restatement's own error against float64 on the same inputs.
      values (map, per_image, mean): max |err| <= max(4 x yardstick, 1e-6)
      gradient: rel-L2 <= max(4 x yardstick, 1e-4), the project's bound (tests/test_ray_grad_host.py)
      gradient, absolute (for the elements whose true gradient is 0 -- the surround-only pixels, x is y -- where a relative figure
        says nothing): max |err| <= max(4 x yardstick's max |err|, 1e-4 x max |gradient|): the same 1e-4, taken of the largest
        element of the case's gradient instead of its norm"""
    if case not in _references:
        x, y = make(case)
        mean, per, smap = (t.detach() for t in ssim64(x.double(), y.double()))
        grad = ssim64_grad(x, y)
        m32, p32, s32 = (t.detach().double() for t in ssim32_torch(x, y))
        g32 = ssim32_torch_grad(x, y).double()
        _references[case] = dict(
            x=x, y=y, mean=mean, per_image=per, map=smap, grad=grad,
            bound_map=max(4.0 * float((s32 - smap).abs().max()), 1e-6),
            bound_per_image=max(4.0 * float((p32 - per).abs().max()), 1e-6),
            bound_mean=max(4.0 * float((m32 - mean).abs()), 1e-6),
            bound_grad_rel=max(4.0 * rel_l2(g32, grad), 1e-4),
            bound_grad_abs=max(4.0 * float((g32 - grad).abs().max()), 1e-4 * float(grad.abs().max())))
    return _references[case]
