"""Environment-map background behind the grid over libvoxe_hip.so: a learned colour that depends on the ray
direction only, composited behind a finished render with the ray's leftover transmittance 1 - acc.  No workspace; reached through
voxe_hip.ops, which re-exports every name here."""
import ctypes as C
from typing import Optional

import torch

from . import abi
from .args import _require_buffer
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr
from .workspace import wrote

MERGE_SHIPPED, MERGE_RUNS, MERGE_PLAIN = 0, 1, 2   # voxe_background_debug_merge


def _env_map(texels: torch.Tensor) -> abi.VoxeEnvMap:
    env = abi.VoxeEnvMap()
    env.texels, env.height, env.width = texels.data_ptr(), int(texels.shape[0]), int(texels.shape[1])
    return env


def _check_inputs(entry: str, texels, rays_d, acc, **colours) -> int:
    """texels [He,We,3], rays_d [R,3], acc [R] / [R,1] and colour tensors [R,3]: contiguous float32 on one GPU; -> R"""
    require_device(texels, f"{entry} (texels)")
    if texels.dim() != 3 or texels.shape[2] != 3 or texels.shape[0] < 2 or texels.shape[1] < 2:
        raise VoxeError(f"{entry}: texels must be [He,We,3] with He >= 2 and We >= 2; got {tuple(texels.shape)}")
    device = texels.device
    _require_buffer(entry, "texels", texels, device=device)
    if rays_d.dim() != 2 or rays_d.shape[1] != 3:
        raise VoxeError(f"{entry}: rays_d must be flat [R,3]; got {tuple(rays_d.shape)}")
    R = int(rays_d.shape[0])
    _require_buffer(entry, "rays_d", rays_d, device=device)
    _require_buffer(entry, "acc", acc, numel=R, device=device)
    for name, t in colours.items():
        _require_buffer(entry, name, t, shape=(R, 3), device=device)
    return R


@torch.no_grad()
def background_fwd_into(texels: torch.Tensor, rays_d: torch.Tensor, colour_in: torch.Tensor, acc: torch.Tensor,
                        colour_out: torch.Tensor) -> None:
    """voxe_background_fwd as it stands: colour_out [R,3] = colour_in + (1 - acc) sigmoid(bilinear(texels at rays_d)); every
    tensor a contiguous float32 buffer on one GPU, `colour_out` may be `colour_in`."""
    R = _check_inputs("background_fwd_into", texels, rays_d, acc, colour_in=colour_in, colour_out=colour_out)
    device = texels.device
    ensure_gfx950(device)
    env = _env_map(texels)
    with torch.cuda.device(device):
        check(lib().voxe_background_fwd(C.byref(env), ptr(rays_d), R, ptr(colour_in), ptr(acc), ptr(colour_out),
                                        stream_ptr(device)), "voxe_background_fwd")
    wrote(colour_out)


@torch.no_grad()
def background_bwd(texels: torch.Tensor, rays_d: torch.Tensor, acc: torch.Tensor, d_colour_out: torch.Tensor,
                   want_acc: bool = True, want_texels: bool = True, want_rays_d: bool = True,
                   d_acc: Optional[torch.Tensor] = None, d_texels: Optional[torch.Tensor] = None,
                   d_rays_d: Optional[torch.Tensor] = None, accumulate: bool = False, merge: int = MERGE_SHIPPED):
    """voxe_background_bwd as it stands: (d_acc [R], d_texels [He,We,3], d_rays_d [R,3]) for the upstream gradient d_colour_out
    [R,3]; want_* = False skips that output (None: its pointer is NULL).  d_acc / d_texels / d_rays_d: caller's buffers, added to
    when `accumulate`.  `merge` (test aid): MERGE_RUNS / MERGE_PLAIN pins how the texel gradient is deposited for this call."""
    R = _check_inputs("background_bwd", texels, rays_d, acc, d_colour_out=d_colour_out)
    device = texels.device
    for name, t, shape in (("d_acc", d_acc, None), ("d_texels", d_texels, texels.shape), ("d_rays_d", d_rays_d, (R, 3))):
        if t is not None:
            _require_buffer("background_bwd", name, t, shape=shape, numel=R if shape is None else None, device=device)
    ensure_gfx950(device)
    env = _env_map(texels)
    L = lib()
    with torch.cuda.device(device):
        if d_acc is None and want_acc:
            d_acc = torch.empty((R,), dtype=torch.float32, device=device)
        if d_texels is None and want_texels:
            d_texels = torch.empty_like(texels)
        if d_rays_d is None and want_rays_d:
            d_rays_d = torch.empty((R, 3), dtype=torch.float32, device=device)
        if R == 0 and d_texels is not None and not accumulate:
            d_texels.zero_()   # (the library touches no output of a call without rays)
        if merge:
            check(L.voxe_background_debug_merge(int(merge)), "voxe_background_debug_merge")
        try:
            check(L.voxe_background_bwd(C.byref(env), ptr(rays_d), R, ptr(acc), ptr(d_colour_out), ptr(d_acc), ptr(d_texels),
                                        ptr(d_rays_d), 1 if accumulate else 0, stream_ptr(device)), "voxe_background_bwd")
        finally:
            if merge:
                L.voxe_background_debug_merge(0)
    wrote(d_acc, d_texels, d_rays_d)
    return d_acc, d_texels, d_rays_d


class _BackgroundFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colour, acc, rays_d, texels, merge):
        for name, t in (("colour", colour), ("acc", acc), ("rays_d", rays_d), ("texels", texels)):
            require_device(t, f"background_composite ({name})")
        col, a, rd, tex = f32c(colour.detach()), f32c(acc.detach()), f32c(rays_d.detach()), f32c(texels.detach())
        out = torch.empty_like(col)
        background_fwd_into(tex, rd, col, a, out)
        ctx.merge = merge
        ctx.save_for_backward(a, rd, tex)
        return out

    @staticmethod
    def backward(ctx, g):
        a, rd, tex = ctx.saved_tensors
        need_c, need_a, need_d, need_t = ctx.needs_input_grad[:4]
        g = f32c(g)
        d_acc = d_tex = d_rd = None
        if need_a or need_d or need_t:
            d_acc, d_tex, d_rd = background_bwd(tex, rd, a, g, want_acc=bool(need_a), want_texels=bool(need_t),
                                                want_rays_d=bool(need_d), merge=ctx.merge)
            if d_acc is not None:
                d_acc = d_acc.reshape(a.shape)
        return (g if need_c else None), d_acc, d_rd, d_tex, None


def background_composite(colour: torch.Tensor, acc: torch.Tensor, rays_d: torch.Tensor, texels: torch.Tensor,
                         _merge: int = MERGE_SHIPPED) -> torch.Tensor:
    """colour [R,3] + (1 - acc) * sigmoid(bilinear(texels [He,We,3] at the direction rays_d [R,3])): the environment map behind a
    render whose colour and accumulated weight acc ([R] or [R,1]) are given.  Longitude wraps, the poles clamp (include/voxe.h).
    Differentiable w.r.t. all four inputs; a gradient that is not needed is not computed."""
    if colour.dim() != 2 or colour.shape[1] != 3 or rays_d.shape != colour.shape or acc.numel() != colour.shape[0]:
        raise VoxeError(f"background_composite: colour and rays_d must be [R,3] and acc hold R values; got {tuple(colour.shape)}, "
                        f"{tuple(rays_d.shape)}, {tuple(acc.shape)}")
    return _BackgroundFn.apply(colour, acc, rays_d, texels, int(_merge))
