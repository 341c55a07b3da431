"""Argument preparation shared by the entry points of voxe_hip.ops and its feature modules (cameras, losses, gridops): the checks
and small conversions every binding of a library call repeats."""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import abi
from . import dispatch as _dispatch
from .runtime import VoxeError, require_device


@dataclass(frozen=True)
class GridSpec:
    """Static (non-tensor) description of a voxel grid: what VoxeGridDesc needs besides pointers."""
    aabb: Tuple[Tuple[float, float], Tuple[float, float], Tuple[float, float]]
    density_scale: float = 1.0
    density_pre_act: int = abi.ACT_IDENTITY
    density_post_act: int = abi.ACT_SOFTPLUS
    feature_kind: int = abi.FEAT_SH


@dataclass
class RenderParams:
    """Everything VoxeRenderCfg holds except the RNG stream and the packed-grid reuse flag."""
    num_samples: int
    near: float
    far: float
    perturb: bool = False
    linear_disparity: bool = False
    aabb_clip: bool = False
    white_bkgd: bool = False
    sh_degree: int = 0
    render_diffuse: bool = False
    term_eps: float = 0.0
    image_width: int = 0
    image_height: int = 0     # > 0 (with image_width): the rays are K = R / (H * W) images, one after the other
    deterministic: bool = False   # backward in 64-bit fixed point: bit-reproducible (test / race-check mode)
    linear_grad: bool = False     # render_bwd_acc: write VOXE_GRAD_LINEAR whatever kernel runs (deferred-gradient mode)
    dispatch: Optional[_dispatch.Dispatch] = None   # kernel routes / tuning of THIS call (VoxeDispatch); None = dispatch.current()


def _next_rng():
    """(seed, offset) of the in-kernel counter-hash jitter stream, tied to torch's CPU generator so that
    torch.manual_seed() makes renders reproducible (no device sync involved)."""
    seed = torch.initial_seed() & 0xFFFFFFFFFFFFFFFF
    offset = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    return seed, offset


def resolve_rng(params, jitter, rng):
    """the (seed, offset) a sampling entry point uses: the caller's `rng`, or -- render's rule -- a fresh stream when the call
    perturbs its samples and no jitter tensor is given, else (0, 0)"""
    if rng is not None:
        return rng
    return _next_rng() if (params.perturb and jitter is None) else (0, 0)


def _check_rays(entry: str, rays_o, rays_d, jitter, num_samples: int) -> None:
    """flat rays [R,3] on the device and, when given, a jitter tensor [R,S]"""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d)):
        require_device(t, f"{entry} ({name})")
    if rays_o.dim() != 2 or rays_o.shape[1] != 3 or rays_o.shape != rays_d.shape:
        raise VoxeError(f"rays must be flat [R,3]; got {tuple(rays_o.shape)}, {tuple(rays_d.shape)}")
    if jitter is not None and tuple(jitter.shape) != (rays_o.shape[0], num_samples):
        raise VoxeError(f"jitter must be [R,S]={rays_o.shape[0], num_samples}; got {tuple(jitter.shape)}")


def _require_buffer(entry: str, name: str, t, *, shape=None, numel=None, device=None, dtype=torch.float32) -> None:
    """a caller's tensor the library reads or writes through its raw pointer: on a GPU (`device`: on that one), contiguous, of
    `dtype` and of the given shape and / or number of elements"""
    if not t.is_cuda:
        require_device(t, f"{entry} ({name})")
    if (t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape))
            or (numel is not None and t.numel() != numel) or (device is not None and t.device != device)):
        want = ", ".join(f"{k} {v}" for k, v in (("shape", shape and tuple(shape)), ("elements", numel), ("on", device)) if v is not None)
        raise VoxeError(f"{entry}: {name} must be a contiguous {dtype} buffer ({want or 'any size'}); "
                        f"got {tuple(t.shape)} {t.dtype} on {t.device}")


def _moments(state):
    """(exp_avg, exp_avg_sq) of an Adam state, (None, None) for a frozen tensor"""
    return state if state is not None else (None, None)
