"""Ray casting over libvoxe_hip.so: rays of pinhole and real-capture cameras, their backward to poses, focal length, intrinsics and
lens distortion, and the pixel-subset draw.  No workspace; reached through voxe_hip.ops, which re-exports every name here."""
import ctypes as C
from typing import Optional, Tuple

import torch

from . import abi
from .args import _next_rng, _require_buffer
from .runtime import VoxeError, check, ensure_gfx950, f32c, lib, ptr, require_device, stream_ptr
from .workspace import _scratch_for


def cast_rays(height: int, width: int, focal: float, rotation, translation, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [H*W,3] on `device` (thre3d_atom/rendering/volumetric/utils/misc.py:12-50)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VoxeError("cast_rays runs on the GPU only (no CPU fallback in the product path)")
    ensure_gfx950(device)
    rot = torch.as_tensor(rotation).detach().to("cpu", torch.float32).reshape(9).contiguous()
    tr = torch.as_tensor(translation).detach().to("cpu", torch.float32).reshape(3).contiguous()
    fp = C.POINTER(C.c_float)
    n = int(height) * int(width)
    with torch.cuda.device(device):
        ro = torch.empty((n, 3), dtype=torch.float32, device=device)
        rd = torch.empty((n, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays(int(height), int(width), float(focal), C.cast(rot.data_ptr(), fp),
                                   C.cast(tr.data_ptr(), fp), ptr(ro), ptr(rd), stream_ptr(device)),
              "voxe_cast_rays")
    return ro, rd


def cast_rays_indexed(height: int, width: int, focal: float, poses: torch.Tensor,
                      flat_index: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rays of selected pixels of K cameras: poses [K,3,4] and flat_index int64 [B] = (camera*H + y)*W + x, both on
    the GPU; -> rays_o, rays_d [B,3].  No host synchronisation, no full-image ray buffers."""
    require_device(poses, "cast_rays_indexed")
    require_device(flat_index, "cast_rays_indexed")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or flat_index.dtype != torch.int64 or flat_index.dim() != 1:
        raise VoxeError("cast_rays_indexed: poses must be [K,3,4] float, flat_index int64 [B]")
    device = poses.device
    ensure_gfx950(device)
    p = f32c(poses)
    idx = flat_index.contiguous()
    n = int(idx.shape[0])
    with torch.cuda.device(device):
        ro = torch.empty((n, 3), dtype=torch.float32, device=device)
        rd = torch.empty((n, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays_indexed(int(height), int(width), float(focal), ptr(p), int(p.shape[0]), ptr(idx), n,
                                           ptr(ro), ptr(rd), stream_ptr(device)), "voxe_cast_rays_indexed")
    return ro, rd


def random_subset(n: int, count: int, device, rng: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """`count` distinct pseudo-random indices of [0, n) (int64, random order) -- the role of torch.randperm(n)[:count]
    without permuting all n.  Reproducible: (seed, counter) come from torch's CPU generator state like the jitter."""
    device = torch.device(device)
    if device.type != "cuda":
        raise VoxeError("random_subset runs on the GPU only (no CPU fallback in the product path)")
    ensure_gfx950(device)
    seed, offset = rng if rng is not None else _next_rng()
    with torch.cuda.device(device):
        out = torch.empty((int(count),), dtype=torch.int64, device=device)
        check(lib().voxe_random_subset(int(n), int(count), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), ptr(out),
                                       stream_ptr(device)), "voxe_random_subset")
    return out


def cast_rays_bwd(height: int, width: int, focal: float, poses: torch.Tensor, flat_index: Optional[torch.Tensor],
                  g_rays_o: Optional[torch.Tensor], g_rays_d: Optional[torch.Tensor], want_focal: bool = False,
                  d_poses: Optional[torch.Tensor] = None, d_focal: Optional[torch.Tensor] = None, accumulate: bool = False):
    """voxe_cast_rays_bwd: (d_poses [K,3,4], d_focal [] or None) of the rays cast_rays_indexed(height, width, focal, poses,
    flat_index) returns -- flat_index None: the K whole images, ray i = pixel i -- for the upstream gradients g_rays_o / g_rays_d
    [B,3] (either may be None = 0).  d_poses / d_focal: caller's buffers, added to when `accumulate`."""
    p, K, idx, B = _camera_call_inputs("cast_rays_bwd", poses, flat_index, height, width, guard_empty_index=False)
    device = p.device
    ups = _upstream_rays("cast_rays_bwd", g_rays_o, g_rays_d, B)
    L = lib()
    with torch.cuda.device(device):
        if d_poses is None:
            d_poses = torch.empty((K, 3, 4), dtype=torch.float32, device=device)
        if d_focal is None and want_focal:
            d_focal = torch.empty((), dtype=torch.float32, device=device)
        sc = _scratch_for(device, L.voxe_cast_rays_bwd_scratch_bytes(K))
        check(L.voxe_cast_rays_bwd(int(height), int(width), float(focal), ptr(p), K, ptr(idx), B, ptr(ups[0]), ptr(ups[1]),
                                   ptr(d_poses), ptr(d_focal), 1 if accumulate else 0, ptr(sc), sc.numel(), stream_ptr(device)),
              "voxe_cast_rays_bwd")
    return d_poses, d_focal


class _CastRaysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, focal_tensor, flat_index, height, width, focal):
        ctx.set_materialize_grads(False)
        if flat_index is None:
            # whole images through the indexed kernel: per pixel the arithmetic of voxe_cast_rays, bit for bit
            index = torch.arange(poses.shape[0] * height * width, dtype=torch.int64, device=poses.device)
        else:
            index = flat_index
        ro, rd = cast_rays_indexed(height, width, focal, poses.detach(), index)
        ctx.save_for_backward(poses, flat_index)
        ctx.geometry = (height, width, focal)
        ctx.focal_like = focal_tensor
        return ro, rd

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, flat_index = ctx.saved_tensors
        height, width, focal = ctx.geometry
        want_focal = ctx.focal_like is not None and ctx.needs_input_grad[1]
        if not (ctx.needs_input_grad[0] or want_focal) or (g_o is None and g_d is None):
            return (None,) * 6
        d_poses, d_focal = cast_rays_bwd(height, width, focal, poses, flat_index, g_o, g_d, want_focal=want_focal)
        if want_focal:
            d_focal = d_focal.to(device=ctx.focal_like.device, dtype=ctx.focal_like.dtype).reshape(ctx.focal_like.shape)
        return (d_poses.to(poses.dtype) if ctx.needs_input_grad[0] else None), (d_focal if want_focal else None), None, None, None, None


def cast_rays_from_poses(height: int, width: int, focal, poses: torch.Tensor,
                         flat_index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [B,3] of poses [K,3,4] (rotation | translation, on the GPU), differentiable w.r.t. `poses` and, when
    `focal` is a 0-dim tensor, w.r.t. the focal length.  flat_index (int64 [B], (camera * H + y) * W + x) picks pixels as
    cast_rays_indexed does; None: the K whole images one after the other.  The forward's bits are those of cast_rays /
    cast_rays_indexed."""
    require_device(poses, "cast_rays_from_poses")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise VoxeError("cast_rays_from_poses: poses must be [K,3,4]")
    focal_tensor = focal if isinstance(focal, torch.Tensor) else None
    if focal_tensor is not None and focal_tensor.dim() != 0:
        raise VoxeError("cast_rays_from_poses: focal must be a number or a 0-dim tensor")
    value = float(focal) if focal_tensor is None else float(focal_tensor.detach())
    return _CastRaysFn.apply(poses, focal_tensor, flat_index, int(height), int(width), value)


# ------------------------------------------------------------------------------------------------
# real-capture cameras: intrinsics + lens distortion
# ------------------------------------------------------------------------------------------------
def _camera_struct(camera, intrinsics=None) -> abi.VoxeCamera:
    """abi.VoxeCamera of `camera`: an abi.VoxeCamera, or any object with height, width, fx, fy, cx, cy and distortion (k1 k2 p1 p2
    k3) such as thre3d_atom's PinholeCamera, or a plain (height, width, focal) tuple (centred, no distortion).  `intrinsics`
    (4 numbers fx fy cx cy) replaces the camera's own."""
    if isinstance(camera, abi.VoxeCamera):
        c = abi.VoxeCamera.from_buffer_copy(camera)
    elif hasattr(camera, "fx"):
        k = [float(v) for v in camera.distortion] + [0.0] * 5
        c = abi.VoxeCamera(int(camera.height), int(camera.width), float(camera.fx), float(camera.fy), float(camera.cx),
                           float(camera.cy), *k[:5])
    else:
        height, width, focal = camera
        c = abi.VoxeCamera(int(height), int(width), float(focal), float(focal), int(width) * 0.5, int(height) * 0.5, 0, 0, 0, 0, 0)
    if intrinsics is not None:
        c.fx, c.fy, c.cx, c.cy = (float(v) for v in intrinsics)
    return c


def _camera_call_inputs(name: str, poses: torch.Tensor, flat_index: Optional[torch.Tensor], height: int, width: int, *,
                        guard_empty_index: bool):
    """(poses as dense float32, K, flat_index or None, B) of a ray-casting call over K cameras of height x width pixels.
    `guard_empty_index` (the camera entries): an empty index is handed over as one unread element."""
    require_device(poses, name)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise VoxeError(f"{name}: poses must be [K,3,4]")
    ensure_gfx950(poses.device)
    p = f32c(poses.detach())
    K = int(p.shape[0])
    if flat_index is not None:
        require_device(flat_index, name)
        if flat_index.dtype != torch.int64 or flat_index.dim() != 1:
            raise VoxeError(f"{name}: flat_index must be int64 [B]")
        idx = flat_index.contiguous()
        B = int(idx.shape[0])
        if B == 0 and guard_empty_index:   # (an empty tensor has no address, and a NULL index means whole images)
            idx = torch.zeros((1,), dtype=torch.int64, device=p.device)
    else:
        idx, B = None, K * int(height) * int(width)
    return p, K, idx, B


def _upstream_rays(name: str, g_rays_o: Optional[torch.Tensor], g_rays_d: Optional[torch.Tensor], B: int):
    """[g_rays_o, g_rays_d] as dense float32 [B,3] (None stays None = 0)"""
    ups = []
    for which, t in (("g_rays_o", g_rays_o), ("g_rays_d", g_rays_d)):
        if t is not None:
            require_device(t, f"{name} ({which})")
            if tuple(t.shape) != (B, 3):
                raise VoxeError(f"{name}: {which} must be [B,3]={B, 3}; got {tuple(t.shape)}")
            t = f32c(t.detach())
        ups.append(t)
    return ups


def cast_rays_camera(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor] = None,
                     intrinsics=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """voxe_cast_rays_camera: rays_o, rays_d [B,3] of `camera` (see _camera_struct) at poses [K,3,4] (GPU).  flat_index (int64
    [B], (camera * H + y) * W + x) picks pixels; None: the K whole images one after the other."""
    cam = _camera_struct(camera, intrinsics)
    p, K, idx, B = _camera_call_inputs("cast_rays_camera", poses, flat_index, cam.H, cam.W, guard_empty_index=True)
    device = p.device
    with torch.cuda.device(device):
        ro = torch.empty((B, 3), dtype=torch.float32, device=device)
        rd = torch.empty((B, 3), dtype=torch.float32, device=device)
        check(lib().voxe_cast_rays_camera(C.byref(cam), ptr(p), K, ptr(idx), B, ptr(ro), ptr(rd), stream_ptr(device)),
              "voxe_cast_rays_camera")
    return ro, rd


def cast_rays_camera_bwd(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor], g_rays_o: Optional[torch.Tensor],
                         g_rays_d: Optional[torch.Tensor], want_poses: bool = True, want_intrinsics: bool = False,
                         want_distortion: bool = False, d_poses: Optional[torch.Tensor] = None,
                         d_intrinsics: Optional[torch.Tensor] = None, d_distortion: Optional[torch.Tensor] = None,
                         accumulate: bool = False, intrinsics=None):
    """voxe_cast_rays_camera_bwd: (d_poses [K,3,4], d_intrinsics [4] fx fy cx cy, d_distortion [5] k1 k2 p1 p2 k3) of the rays
    cast_rays_camera(camera, poses, flat_index) returns, for the upstream gradients g_rays_o / g_rays_d [B,3] (either may be None
    = 0).  An output is None unless wanted or given as the caller's buffer, which is added to when `accumulate`."""
    cam = _camera_struct(camera, intrinsics)
    p, K, idx, B = _camera_call_inputs("cast_rays_camera_bwd", poses, flat_index, cam.H, cam.W, guard_empty_index=True)
    device = p.device
    ups = _upstream_rays("cast_rays_camera_bwd", g_rays_o, g_rays_d, B)
    for name, t, shape in (("d_poses", d_poses, (K, 3, 4)), ("d_intrinsics", d_intrinsics, (4,)), ("d_distortion", d_distortion, (5,))):
        if t is not None:
            _require_buffer("cast_rays_camera_bwd", name, t, shape=shape)
    L = lib()
    with torch.cuda.device(device):
        if d_poses is None and want_poses:
            d_poses = torch.empty((K, 3, 4), dtype=torch.float32, device=device)
        if d_intrinsics is None and want_intrinsics:
            d_intrinsics = torch.empty((4,), dtype=torch.float32, device=device)
        if d_distortion is None and want_distortion:
            d_distortion = torch.empty((5,), dtype=torch.float32, device=device)
        sc = _scratch_for(device, L.voxe_cast_rays_camera_bwd_scratch_bytes(K))
        check(L.voxe_cast_rays_camera_bwd(C.byref(cam), ptr(p), K, ptr(idx), B, ptr(ups[0]), ptr(ups[1]), ptr(d_poses),
                                          ptr(d_intrinsics), ptr(d_distortion), 1 if accumulate else 0, ptr(sc), sc.numel(),
                                          stream_ptr(device)), "voxe_cast_rays_camera_bwd")
    return d_poses, d_intrinsics, d_distortion


class _CastRaysCameraFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, poses, intrinsics, distortion, flat_index, cam):
        ctx.set_materialize_grads(False)
        from . import ops   # (at call time: `ops.cast_rays_camera` is the name callers -- and tests -- may replace)

        ro, rd = ops.cast_rays_camera(cam, poses.detach(), flat_index)
        ctx.save_for_backward(poses, flat_index)
        ctx.cam = cam
        ctx.like = [None if t is None else (t.device, t.dtype, t.shape) for t in (intrinsics, distortion)]
        return ro, rd

    @staticmethod
    def backward(ctx, g_o, g_d):
        poses, flat_index = ctx.saved_tensors
        want = [bool(n) for n in ctx.needs_input_grad[:3]]
        if not any(want) or (g_o is None and g_d is None):
            return (None,) * 5
        outs = cast_rays_camera_bwd(ctx.cam, poses, flat_index, g_o, g_d, want_poses=want[0], want_intrinsics=want[1],
                                    want_distortion=want[2])
        grads = [outs[0].to(poses.dtype) if want[0] else None]
        for got, like, w in zip(outs[1:], ctx.like, want[1:]):
            grads.append(got.to(device=like[0], dtype=like[1]).reshape(like[2]) if w else None)
        return (*grads, None, None)


def cast_rays_from_camera(camera, poses: torch.Tensor, flat_index: Optional[torch.Tensor] = None,
                          intrinsics: Optional[torch.Tensor] = None,
                          distortion: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """rays_o, rays_d [B,3] of `camera` at poses [K,3,4] (GPU), differentiable w.r.t. `poses` and the optional tensors
    `intrinsics` [4] (fx fy cx cy) and `distortion` [5] (k1 k2 p1 p2 k3), whose VALUES replace the camera's own.  The forward's
    bits are those of cast_rays_camera.  The camera travels by value in the call's arguments, so the two tensors are read on the
    host: keep them there (as LearnedIntrinsics does), a device tensor costs a synchronisation per call."""
    cam = _camera_struct(camera)
    if intrinsics is not None:
        if not isinstance(intrinsics, torch.Tensor) or tuple(intrinsics.shape) != (4,):
            raise VoxeError("cast_rays_from_camera: intrinsics must be a tensor [4] = fx fy cx cy")
        cam.fx, cam.fy, cam.cx, cam.cy = (float(v) for v in intrinsics.detach().cpu())
    if distortion is not None:
        if not isinstance(distortion, torch.Tensor) or tuple(distortion.shape) != (5,):
            raise VoxeError("cast_rays_from_camera: distortion must be a tensor [5] = k1 k2 p1 p2 k3")
        cam.k1, cam.k2, cam.p1, cam.p2, cam.k3 = (float(v) for v in distortion.detach().cpu())
    require_device(poses, "cast_rays_from_camera")
    return _CastRaysCameraFn.apply(poses, intrinsics, distortion, flat_index, cam)
