"""What the real-capture importers share (tools/convert_from_colmap_text.py, tools/convert_from_nerfstudio_transforms.py):
the camera-parameter entries of this project's `<split>_camera_params.json`, re-centring, and bounds from a point cloud.
Standard library + numpy only.

Convention of this project: camera-to-world [R | t], camera axes x right, y up, looking down -z (OpenGL)."""
import json
from pathlib import Path

import numpy as np

KEYS = dict(intrinsic="intrinsic", extrinsic="extrinsic", bounds="bounds", height="height", width="width", focal="focal",
            rotation="rotation", translation="translation", fx="fx", fy="fy", cx="cx", cy="cy", distortion="distortion")


def optical_axes_meeting_point(rotations, centres):
    """least-squares point closest to all optical axes (lines through centre c_i along -z_i): solves
    sum (I - d d^T) p = sum (I - d d^T) c"""
    A, b = np.zeros((3, 3)), np.zeros(3)
    for R, c in zip(rotations, centres):
        d = -np.asarray(R, np.float64)[:, 2]
        M = np.eye(3) - np.outer(d, d)
        A += M
        b += M @ np.asarray(c, np.float64)
    return np.linalg.lstsq(A, b, rcond=None)[0]


def depth_bounds(rotation, centre, points, lo=1.0, hi=99.0):
    """(near, far): the lo-th / hi-th percentile of the depths (along the viewing direction) of `points` [N,3] in front of the camera"""
    depth = (np.asarray(points, np.float64) - np.asarray(centre, np.float64)) @ -np.asarray(rotation, np.float64)[:, 2]
    depth = depth[depth > 0]
    if depth.size == 0:
        raise ValueError("no 3D point lies in front of a camera: cannot derive its bounds")
    return float(np.percentile(depth, lo)), float(np.percentile(depth, hi))


def entry(height, width, fx, fy, cx, cy, distortion, rotation, centre, near, far):
    k = KEYS
    return {
        k["intrinsic"]: {k["bounds"]: [float(near), float(far)], k["height"]: int(height), k["width"]: int(width),
                         k["focal"]: float(fx), k["fx"]: float(fx), k["fy"]: float(fy), k["cx"]: float(cx), k["cy"]: float(cy),
                         k["distortion"]: [float(v) for v in distortion]},
        k["extrinsic"]: {k["rotation"]: [[float(v) for v in row] for row in np.asarray(rotation)],
                         k["translation"]: [[float(v)] for v in np.asarray(centre).reshape(3)]},
    }


def write_params(output_path, split, entries) -> Path:
    out = Path(output_path)
    out.mkdir(parents=True, exist_ok=True)
    path = out / f"{split}_camera_params.json"
    path.write_text(json.dumps(entries, indent=2))
    return path
