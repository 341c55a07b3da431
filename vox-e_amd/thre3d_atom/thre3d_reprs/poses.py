"""Learnable camera-pose corrections (DESIGN.md section 4 "Ray gradients").  Not in the reference.

A camera-to-world pose [R | t] is corrected by a rotation exp(w^) applied on the left and a translation tau added:
[exp(w^) R | t + tau], with (w, tau) six numbers per camera that start at zero.  Rays cast from the corrected poses by
voxe_hip.ops.cast_rays_from_poses carry the render's gradient back to them (voxe_render_bwd_rays -> voxe_cast_rays_bwd), which
is what pose refinement while training (BARF, NeRF--) and registering a photograph against a trained grid (iNeRF) need.
The six numbers per camera are tiny tensors: their arithmetic is plain torch, the per-ray work is in the HIP library."""
import json
import math
from pathlib import Path
from typing import Optional

import torch
from torch import Tensor

from thre3d_atom.data.constants import BOUNDS, EXTRINSIC, HEIGHT, INTRINSIC, ROTATION, TRANSLATION, WIDTH


def _hat(w: Tensor) -> Tensor:
    """[N,3] -> [N,3,3] cross-product matrices"""
    zero = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([zero, -w[:, 2], w[:, 1]], dim=1),
                        torch.stack([w[:, 2], zero, -w[:, 0]], dim=1),
                        torch.stack([-w[:, 1], w[:, 0], zero], dim=1)], dim=1)


def axis_angle_to_matrix(w: Tensor) -> Tensor:
    """Rodrigues: exp(w^) = I + A w^ + B w^ w^, A = sin(t) / t, B = (1 - cos t) / t^2, t = |w|.  Below t^2 = 1e-8 the two
    coefficients are their Taylor series in t^2 (1 - t^2/6, 1/2 - t^2/24), which makes the map smooth -- and its gradient
    finite -- at w = 0, where the deltas start."""
    t2 = (w * w).sum(dim=1)
    small = t2 < 1e-8
    safe = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(safe)
    A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(t) / t)
    B = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(t)) / safe)
    K = _hat(w)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand(w.shape[0], 3, 3)
    return eye + A[:, None, None] * K + B[:, None, None] * (K @ K)


class CameraPoseDeltas(torch.nn.Module):
    """One (axis-angle w, translation tau) per camera, [N,6], initialised to zero (the identity correction)."""

    def __init__(self, num_cameras: int):
        super().__init__()
        self.deltas = torch.nn.Parameter(torch.zeros(int(num_cameras), 6))

    def apply(self, poses: Tensor, indices: Optional[Tensor] = None) -> Tensor:   # noqa: A003 (the issue's name)
        """poses [K,3,4] of the cameras `indices` (int64 [K]; None: all N, in order) -> [exp(w^) R | t + tau]"""
        if not isinstance(poses, Tensor):   # nn.Module.apply(fn): the base class's meaning for callables stays
            return super().apply(poses)
        d = self.deltas if indices is None else self.deltas[indices]
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] != d.shape[0]:
            raise ValueError(f"poses must be [K,3,4] with one row of deltas each; got {tuple(poses.shape)} for {d.shape[0]} cameras")
        d = d.to(poses.dtype)
        rot = axis_angle_to_matrix(d[:, :3]) @ poses[:, :, :3]
        return torch.cat([rot, poses[:, :, 3:] + d[:, 3:, None]], dim=2)

    forward = apply


class LearnedIntrinsics(torch.nn.Module):
    """fx, fy, cx, cy of the one shared camera as a parameter [4] (pixels), started at the camera's own; the distortion
    coefficients stay fixed (learning them is out of scope).  Rays cast by voxe_hip.ops.cast_rays_from_camera(camera, poses,
    index, intrinsics=self.values) carry the render's gradient back to it (voxe_cast_rays_camera_bwd).  The parameter lives on
    the HOST: the camera is passed to the kernels by value, so a device tensor would cost a synchronisation per iteration."""

    def __init__(self, camera_intrinsics):
        super().__init__()
        from thre3d_atom.utils.imaging_utils import PinholeCamera

        if isinstance(camera_intrinsics, PinholeCamera):
            self.base = camera_intrinsics
        else:
            height, width, focal = camera_intrinsics
            self.base = PinholeCamera(height, width, focal)
        self.values = torch.nn.Parameter(torch.tensor([self.base.fx, self.base.fy, self.base.cx, self.base.cy], dtype=torch.float32))

    def camera(self):
        """the PinholeCamera with the learned intrinsics"""
        return self.base.with_intrinsics(*(float(v) for v in self.values.detach().cpu()))


def rotation_error_degrees(poses: Tensor, reference: Tensor) -> Tensor:
    """[K] angle of R_a R_b^T in degrees, poses [K,3,4] or [K,3,3]"""
    rel = poses[:, :, :3].double() @ reference[:, :, :3].double().transpose(1, 2)
    cos = ((rel[:, 0, 0] + rel[:, 1, 1] + rel[:, 2, 2]) - 1.0) * 0.5
    return torch.rad2deg(torch.acos(cos.clamp(-1.0, 1.0)))


def translation_error(poses: Tensor, reference: Tensor) -> Tensor:
    """[K] distance between the camera centres"""
    return (poses[:, :, 3].double() - reference[:, :, 3].double()).norm(dim=1)


def write_camera_params(path, dataset, poses: Tensor, camera=None) -> Path:
    """Write `poses` [N,3,4] (the dataset's cameras, in its order) as a `<split>_camera_params.json` PosedImagesDataset reads.
    A PosedImagesDataset keeps its file names and per-image intrinsics; any other dataset gets 0000.png ... and its own
    intrinsics (a PinholeCamera with its whole model) and bounds.  `camera` (a PinholeCamera at the FILE's image size, e.g.
    refined intrinsics) replaces the camera model of every entry."""
    from thre3d_atom.data.datasets import CAMERA_MODEL_KEYS, camera_to_params

    poses = poses.detach().cpu().double()
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] != len(dataset):
        raise ValueError(f"poses must be [{len(dataset)},3,4]; got {tuple(poses.shape)}")
    source = getattr(dataset, "camera_parameters", None)
    if source is not None:
        config = dataset.get_config_dict()
        if config.get("normalize_scene_scale"):
            # the dataset divided every camera location by the distance of the farthest camera of its file: back to file units
            radii = [float(torch.tensor(entry[EXTRINSIC][TRANSLATION], dtype=torch.float32).norm()) for entry in source.values()]
            poses = torch.cat([poses[:, :, :3], poses[:, :, 3:] * max(max(radii), 1e-8)], dim=2)
        files = sorted(p.name for p in Path(config["images_dir"]).iterdir() if p.suffix.lower() in (".png", ".jpg", ".jpeg"))
        names = [n for n in files if n in source] or files
        entries = {n: json.loads(json.dumps(source[n])) for n in names}
    else:
        near, far = dataset.camera_bounds
        width = max(4, int(math.log10(max(len(dataset), 1))) + 1)
        names = [f"{i:0{width}d}.png" for i in range(len(dataset))]
        entries = {n: {EXTRINSIC: {}, INTRINSIC: {**camera_to_params(dataset.camera_intrinsics), BOUNDS: [float(near), float(far)]}}
                   for n in names}
    if camera is not None:
        for entry in entries.values():
            if (int(entry[INTRINSIC][HEIGHT]), int(entry[INTRINSIC][WIDTH])) != (camera.height, camera.width):
                raise ValueError(f"`camera` is {camera.height} x {camera.width}, the file's images are "
                                 f"{entry[INTRINSIC][HEIGHT]} x {entry[INTRINSIC][WIDTH]}")
            for k in CAMERA_MODEL_KEYS:
                entry[INTRINSIC].pop(k, None)
            entry[INTRINSIC].update(camera_to_params(camera))
    if len(names) != poses.shape[0]:
        raise ValueError(f"{len(names)} images for {poses.shape[0]} poses")
    for n, pose in zip(names, poses):
        entries[n][EXTRINSIC][ROTATION] = [[float(x) for x in row] for row in pose[:, :3]]
        entries[n][EXTRINSIC][TRANSLATION] = [[float(x)] for x in pose[:, 3]]
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(entries, indent=2))
    return path
