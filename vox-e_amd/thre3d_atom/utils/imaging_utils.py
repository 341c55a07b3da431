"""Camera tuples, range adjustment and synthetic camera paths.

Mirrors the names of the reference's thre3d_atom/utils/imaging_utils.py.  The numeric conventions
that define index math downstream are kept bit-for-bit:
  * adjust_dynamic_range(slack=True) computes scale and bias in np.float32 (imaging_utils.py:57-63);
  * pose_spherical builds float32 4x4 matrices from float64 sines/cosines and multiplies them in
    float32 in the order yaw @ (pitch @ translate) (imaging_utils.py:188-194).
"""
import math
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from thre3d_atom.utils.constants import NUM_COLOUR_CHANNELS


class CameraIntrinsics(NamedTuple):
    height: int
    width: int
    focal: float


DISTORTION_NAMES = ("k1", "k2", "p1", "p2", "k3")   # OpenCV order
MIN_LENS_JACOBIAN_DET = 0.1    # PinholeCamera.validate(): the lens model must stay monotonic over the image


class PinholeCamera(CameraIntrinsics):
    """A real-capture camera: fx != fy, an off-centre principal point and the OpenCV radial / tangential lens
    model (k1, k2, p1, p2, k3).  Pixel (px, py) has its centre at (px + 0.5, py + 0.5); fx, fy, cx, cy are in pixels.
    It IS a CameraIntrinsics tuple and unpacks to (height, width, focal) with focal = fx, so code that only passes
    `camera_intrinsics` through keeps working; the full model travels as attributes (and through pickle: checkpoints store this
    object).  One camera is shared by all images of a dataset."""

    def __new__(cls, height, width, fx, fy=None, cx=None, cy=None, distortion=None):
        fx = float(fx)
        self = super().__new__(cls, int(height), int(width), fx)
        self.fx, self.fy = fx, float(fx if fy is None else fy)
        self.cx = float(self.width * 0.5 if cx is None else cx)
        self.cy = float(self.height * 0.5 if cy is None else cy)
        coeffs = tuple(float(v) for v in (distortion if distortion is not None else ()))
        if len(coeffs) > len(DISTORTION_NAMES):
            raise ValueError(f"distortion takes at most {len(DISTORTION_NAMES)} coefficients {DISTORTION_NAMES}; got {len(coeffs)}")
        self.distortion = coeffs + (0.0,) * (len(DISTORTION_NAMES) - len(coeffs))
        return self

    def __reduce__(self):
        return (PinholeCamera, (self.height, self.width, self.fx, self.fy, self.cx, self.cy, self.distortion))

    def __repr__(self) -> str:
        return (f"PinholeCamera(height={self.height}, width={self.width}, fx={self.fx}, fy={self.fy}, cx={self.cx}, cy={self.cy}, "
                f"distortion={self.distortion})")

    def _model(self):
        return (tuple(self), self.fy, self.cx, self.cy, self.distortion)

    def __eq__(self, other):
        if isinstance(other, PinholeCamera):
            return self._model() == other._model()
        return self.is_legacy() and tuple(self) == other if isinstance(other, tuple) else NotImplemented

    def __ne__(self, other):
        result = self.__eq__(other)
        return result if result is NotImplemented else not result

    def __hash__(self):
        return hash(self._model())

    @property
    def has_distortion(self) -> bool:
        return any(v != 0.0 for v in self.distortion)

    def is_legacy(self) -> bool:
        """what (height, width, focal) alone describes: centred, square pixels, no distortion"""
        return (self.fx == self.fy and self.cx == self.width * 0.5 and self.cy == self.height * 0.5
                and not self.has_distortion)

    def undistorted(self) -> "PinholeCamera":
        """the same pinhole without its lens: what a novel view is rendered with"""
        return PinholeCamera(self.height, self.width, self.fx, self.fy, self.cx, self.cy)

    def with_intrinsics(self, fx, fy, cx, cy) -> "PinholeCamera":
        return PinholeCamera(self.height, self.width, fx, fy, cx, cy, self.distortion)

    def scaled(self, factor: float) -> "PinholeCamera":
        """the camera of the images resized by 1 / factor: fx, fy, cx, cy divided, height and width TRUNCATED as
        InMemoryPosedImages.downsampled does (800 px / 3.0 -> 266 px); the coefficients act on normalised coordinates and stay"""
        return PinholeCamera(max(int(self.height / factor), 1), max(int(self.width / factor), 1), self.fx / factor,
                             self.fy / factor, self.cx / factor, self.cy / factor, self.distortion)

    def _lens(self, xu, yu):
        """D(xu, yu) and the entries of its symmetric Jacobian, float64"""
        k1, k2, p1, p2, k3 = self.distortion
        xx, yy, xy = xu * xu, yu * yu, xu * yu
        r2 = xx + yy
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        drad = k1 + r2 * (2.0 * k2 + 3.0 * r2 * k3)
        dx = xu * rad + 2.0 * p1 * xy + p2 * (r2 + 2.0 * xx)
        dy = yu * rad + p1 * (r2 + 2.0 * yy) + 2.0 * p2 * xy
        j00 = rad + 2.0 * xx * drad + 2.0 * p1 * yu + 6.0 * p2 * xu
        j01 = 2.0 * xy * drad + 2.0 * p1 * xu + 2.0 * p2 * yu
        j11 = rad + 2.0 * yy * drad + 6.0 * p1 * yu + 2.0 * p2 * xu
        return dx, dy, j00, j01, j11

    def validate(self) -> "PinholeCamera":
        """Raise unless the model can be cast: positive finite focal lengths, finite everything, and a lens model that is
        monotonic over the image.  In float64, for every pixel of the image border (where the polynomial folds first): Newton from
        the pixel's normalised coordinates must reach D(xu, yu) = (xd, yd), and det J must stay >= MIN_LENS_JACOBIAN_DET at the
        start, at the solution and along the segment from the optical axis to the solution.  The ray-casting kernel does not
        check any of this."""
        values = (self.fx, self.fy, self.cx, self.cy) + self.distortion
        if self.height <= 0 or self.width <= 0 or not all(math.isfinite(v) for v in values) or self.fx <= 0 or self.fy <= 0:
            raise ValueError(f"not a camera: {self!r}")
        if not self.has_distortion:
            return self
        xs = (np.arange(self.width) + 0.5 - self.cx) / self.fx
        ys = (np.arange(self.height) + 0.5 - self.cy) / self.fy
        xd = np.concatenate([xs, xs, np.full_like(ys, xs[0]), np.full_like(ys, xs[-1])])
        yd = np.concatenate([np.full_like(xs, ys[0]), np.full_like(xs, ys[-1]), ys, ys])
        xu, yu = xd.copy(), yd.copy()
        lowest = np.inf
        with np.errstate(all="ignore"):
            for _ in range(20):
                dx, dy, j00, j01, j11 = self._lens(xu, yu)
                det = j00 * j11 - j01 * j01
                lowest = min(lowest, float(np.min(det))) if np.all(np.isfinite(det)) else -np.inf
                ex, ey = dx - xd, dy - yd
                xu, yu = xu - (j11 * ex - j01 * ey) / det, yu - (j00 * ey - j01 * ex) / det
            dx, dy, *_ = self._lens(xu, yu)
            residual = float(np.max(np.abs(dx - xd) + np.abs(dy - yd)))
            for t in np.linspace(0.0, 1.0, 17)[1:]:
                _, _, j00, j01, j11 = self._lens(t * xu, t * yu)
                lowest = min(lowest, float(np.min(j00 * j11 - j01 * j01)))
        if not lowest >= MIN_LENS_JACOBIAN_DET:
            raise ValueError(f"the lens model of {self!r} is not invertible over the image: on the image border det of its "
                             f"Jacobian falls to {lowest:.3f} (< {MIN_LENS_JACOBIAN_DET}); undistort the images first")
        if not (np.isfinite(residual) and residual < 1e-9):
            raise ValueError(f"the lens model of {self!r} is not invertible over the image: the undistortion of its border "
                             f"pixels does not converge (residual {residual:.1e}); undistort the images first")
        return self


class CameraPose(NamedTuple):
    rotation: np.array  # [3 x 3]
    translation: np.array  # [3 x 1]


class CameraBounds(NamedTuple):
    near: float
    far: float


def to8b(x: np.array) -> np.array:
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def adjust_dynamic_range(
    data: Union[np.array, Tensor],
    drange_in: Tuple[float, float],
    drange_out: Tuple[float, float],
    slack: bool = False,
):
    """Affine map of `data` from drange_in to drange_out.  slack=True leaves values outside the input
    range un-clipped (this is the form VoxelGrid uses to normalise sample points)."""
    if drange_in == drange_out:
        return data
    in_lo, in_hi = np.float32(drange_in[0]), np.float32(drange_in[1])
    out_lo, out_hi = np.float32(drange_out[0]), np.float32(drange_out[1])
    if slack:
        scale = (out_hi - out_lo) / (in_hi - in_lo)
        bias = out_lo - in_lo * scale
        return data * scale + bias
    data = ((data - in_lo) / (in_hi - in_lo) * (out_hi - out_lo)) + out_lo
    return data.clip(drange_out[0], drange_out[1])


def get_2d_coordinates(height: int, width: int, drange: Tuple[float, float] = (-1.0, 1.0)) -> Tensor:
    lo, hi = drange
    ys = torch.linspace(lo, hi, height, dtype=torch.float32)
    xs = torch.linspace(lo, hi, width, dtype=torch.float32)
    return torch.stack(torch.meshgrid(ys, xs, indexing="ij"), dim=-1)


def postprocess_depth_map(depth_map: np.array, acc_map: Optional[np.array] = None) -> np.array:
    """Depth -> magma colour map, optionally alpha-composited over white using the accumulated weight."""
    import matplotlib.pyplot as plt

    if depth_map.ndim == 3 and depth_map.shape[-1] == 1:
        depth_map = depth_map[..., 0]
    if acc_map is not None:
        lo, hi = depth_map.min(), (depth_map * acc_map[..., 0]).max()
    else:
        lo, hi = depth_map.min(), depth_map.max()
    norm = adjust_dynamic_range(depth_map, drange_in=(lo, hi), drange_out=(0, 1), slack=True)
    coloured = plt.get_cmap("magma", lut=1024)(norm)[..., :NUM_COLOUR_CHANNELS]
    if acc_map is None:
        return to8b(coloured)
    bg = (1.0 - acc_map) ** 2
    return to8b((coloured * acc_map + bg) / (acc_map + bg))


def novel_view_camera(camera_intrinsics: CameraIntrinsics) -> CameraIntrinsics:
    """the camera a NOVEL view (a turntable, a spiral) is rendered with: the dataset's pinhole without its lens.  Views through
    the dataset's real cameras (hold-out evaluation, visibility, pruning) keep the full model."""
    return camera_intrinsics.undistorted() if isinstance(camera_intrinsics, PinholeCamera) else camera_intrinsics


def scale_camera_intrinsics(camera_intrinsics: CameraIntrinsics, scale_factor: float = 1.0) -> CameraIntrinsics:
    if isinstance(camera_intrinsics, PinholeCamera):
        c = camera_intrinsics
        return PinholeCamera(int(np.ceil(c.height * scale_factor)), int(np.ceil(c.width * scale_factor)), c.fx * scale_factor,
                             c.fy * scale_factor, c.cx * scale_factor, c.cy * scale_factor, c.distortion)
    return CameraIntrinsics(
        height=int(np.ceil(camera_intrinsics.height * scale_factor)),
        width=int(np.ceil(camera_intrinsics.width * scale_factor)),
        focal=camera_intrinsics.focal * scale_factor,
    )


# ---------------------------------------------------------------------------------------------
# camera-to-world transforms
# ---------------------------------------------------------------------------------------------
def _mat(rows, device) -> Tensor:
    return torch.tensor(rows, dtype=torch.float32, device=device)


def _translate_z(z: float, device=torch.device("cpu")) -> Tensor:
    return _mat([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, z], [0.0, 0.0, 0.0, 1.0]], device)


def _rotate_pitch(pitch: float, device=torch.device("cpu")) -> Tensor:
    c, s = np.cos(pitch), np.sin(pitch)
    return _mat([[1.0, 0.0, 0.0, 0.0], [0.0, c, -s, 0.0], [0.0, s, c, 0.0], [0.0, 0.0, 0.0, 1.0]], device)


def _rotate_yaw(yaw: float, device=torch.device("cpu")) -> Tensor:
    c, s = np.cos(yaw), np.sin(yaw)
    return _mat([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]], device)


def _spherical_c2w(yaw_deg: float, pitch_deg: float, radius: float, device) -> Tensor:
    c2w = _translate_z(radius, device)
    c2w = _rotate_pitch(pitch_deg / 180.0 * np.pi, device) @ c2w
    return _rotate_yaw(yaw_deg / 180.0 * np.pi, device) @ c2w


def pose_spherical(yaw: float, pitch: float, radius: float, device=torch.device("cpu")) -> CameraPose:
    c2w = _spherical_c2w(yaw, pitch, radius, device)
    return CameraPose(rotation=c2w[:3, :3], translation=c2w[:3, 3:])


def view_direction_label(yaw: float, pitch: float) -> str:
    """Prompt suffix bucket of a random SDS pose (imaging_utils.py:206-213)."""
    label = "front"
    if 45.0 < yaw < 315.0:
        label = "side"
    if 120.0 < yaw < 240.0:
        label = "back"
    if pitch < 25.0:
        label = "overhead"
    return label


def get_random_pose(radius: float, device=torch.device("cpu")):
    """Random SDS camera: pitch ~ U[15, 90), yaw ~ U[0, 360) from numpy's global RNG (two draws, pitch
    first, like imaging_utils.py:197-215).  Returns (pose, direction label, pitch, yaw)."""
    pitch = 15.0 + float(np.random.rand(1)[0] * 75.0)
    yaw = float(np.random.rand(1)[0] * 360.0)
    c2w = _spherical_c2w(yaw, pitch, radius, device)
    pose = CameraPose(rotation=c2w[:3, :3], translation=c2w[:3, 3:])
    return pose, view_direction_label(yaw, pitch), pitch, yaw


def get_thre360_animation_poses(hemispherical_radius: float, camera_pitch: float, num_poses: int) -> Sequence[CameraPose]:
    """num_poses - 1 poses on a circle (the closing duplicate is dropped so a looped video is smooth)."""
    return [pose_spherical(yaw, camera_pitch, hemispherical_radius) for yaw in np.linspace(0, 360, num_poses)[:-1]]


def get_thre360_spiral_animation_poses(
    horizontal_radius_range: Tuple[float, float], vertical_camera_height: float, num_rounds: int, num_poses: int
) -> Sequence[CameraPose]:
    radii = np.linspace(*horizontal_radius_range, num_poses)[:-1]
    yaws = np.linspace(0, 360 * num_rounds, num_poses)[:-1]
    poses = []
    for yaw, r in zip(yaws, radii):
        pitch = math.atan(r / vertical_camera_height) * 180 / math.pi
        poses.append(pose_spherical(yaw, pitch, np.sqrt(r ** 2 + vertical_camera_height ** 2)))
    return poses
