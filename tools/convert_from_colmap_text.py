#!/usr/bin/env python3
"""COLMAP text model (cameras.txt, images.txt, optionally points3D.txt) -> `<split>_camera_params.json` of this project,
with the camera's fx, fy, cx, cy and OpenCV distortion coefficients and, when points3D.txt is there,
`<split>_sparse_points.npz` next to it: the sparse point cloud as per-image depth measurements.

    python tools/convert_from_colmap_text.py -m sparse/0 -o scene [--split train] [--recentre] [--near 0.5 --far 6]

Supported camera models: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV.  The model must hold exactly ONE camera (one
shared camera per dataset).  COLMAP stores world-to-camera (qvec, tvec) with OpenCV axes (x right, y down, looking down +z);
this project wants camera-to-world with x right, y up, looking down -z:  R_c2w = R_w2c^T diag(1, -1, -1),  t = -R_w2c^T tvec.
COLMAP's pixel coordinates put the centre of the top-left pixel at (0.5, 0.5), as this project does, so cx, cy pass unchanged.
Bounds: the 1st / 99th percentile of the depths of the image's own 3D points when points3D.txt is there, else --near / --far.
--recentre moves the least-squares meeting point of the optical axes to the origin.
The sparse-point file (--no_sparse_points suppresses it) holds, for the images in the JSON's order: `names` [K], `offsets` [K+1]
(the observations of image i are rows offsets[i] .. offsets[i+1]), `xy` [M,2] float32 (COLMAP pixel coordinates of the
keypoint), `xyz` [M,3] float32 (the world point, after the --recentre shift) and `error` [M] float32 (the point's mean
reprojection error in pixels).  Observations of points behind the camera or outside the image are dropped.
Standard library + numpy only."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_import as CI  # noqa: E402

# model -> (number of parameters, function of the parameters -> (fx, fy, cx, cy, (k1, k2, p1, p2, k3)))
MODELS = {
    "SIMPLE_PINHOLE": (3, lambda p: (p[0], p[0], p[1], p[2], (0, 0, 0, 0, 0))),
    "PINHOLE": (4, lambda p: (p[0], p[1], p[2], p[3], (0, 0, 0, 0, 0))),
    "SIMPLE_RADIAL": (4, lambda p: (p[0], p[0], p[1], p[2], (p[3], 0, 0, 0, 0))),
    "RADIAL": (5, lambda p: (p[0], p[0], p[1], p[2], (p[3], p[4], 0, 0, 0))),
    "OPENCV": (8, lambda p: (p[0], p[1], p[2], p[3], (p[4], p[5], p[6], p[7], 0))),
}


class UnsupportedModel(ValueError):
    pass


def _lines(path):
    for line in Path(path).read_text().splitlines():
        line = line.strip()
        if line and not line.startswith("#"):
            yield line


def read_camera(path):
    """-> (camera id, width, height, fx, fy, cx, cy, distortion)"""
    cameras = [line.split() for line in _lines(path)]
    if len(cameras) != 1:
        raise UnsupportedModel(f"{path} holds {len(cameras)} cameras: only a model with exactly one shared camera is supported "
                               f"(per-image intrinsics and mixed image sizes are not)")
    cam_id, model, width, height, *params = cameras[0]
    if model not in MODELS:
        raise UnsupportedModel(f"camera model {model} is not supported (supported: {', '.join(MODELS)}); fisheye / equidistant "
                               f"models are out of scope")
    count, unpack = MODELS[model]
    if len(params) != count:
        raise ValueError(f"{model} takes {count} parameters; {path} gives {len(params)}")
    return (int(cam_id), int(width), int(height), *unpack([float(v) for v in params]))


def quaternion_to_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def read_images(path, camera_id):
    """-> [(name, R_c2w, centre, [point3D ids], [(x, y, point3D id)])], sorted by name.  images.txt: two lines per image, the
    second (possibly empty) holding its 2D points; those without a 3D point (id -1) are left out"""
    raw = [line.rstrip("\n") for line in Path(path).read_text().splitlines() if not line.lstrip().startswith("#")]
    while raw and not raw[-1].strip():
        raw.pop()
    out = []
    i = 0
    while i < len(raw):
        if not raw[i].strip():
            i += 1
            continue
        head = raw[i].split()
        points = raw[i + 1].split() if i + 1 < len(raw) else []
        i += 2
        if int(head[8]) != camera_id:
            raise UnsupportedModel(f"image {head[9]} uses camera {head[8]}, not the model's one camera {camera_id}")
        R_w2c = quaternion_to_matrix([float(v) for v in head[1:5]])
        tvec = np.array([float(v) for v in head[5:8]])
        R = R_w2c.T @ np.diag([1.0, -1.0, -1.0])
        centre = -R_w2c.T @ tvec
        ids = [int(v) for v in points[2::3] if int(v) >= 0]
        obs = [(float(x), float(y), int(v)) for x, y, v in zip(points[0::3], points[1::3], points[2::3]) if int(v) >= 0]
        out.append((" ".join(head[9:]), R, centre, ids, obs))
    return sorted(out, key=lambda t: t[0])


def read_points(path):
    return {int(p[0]): np.array([float(v) for v in p[1:4]]) for p in (line.split() for line in _lines(path))}


def read_point_errors(path):
    """point3D id -> mean reprojection error in pixels (POINT3D_ID X Y Z R G B ERROR TRACK[])"""
    return {int(p[0]): float(p[7]) for p in (line.split() for line in _lines(path))}


def sparse_points(model_dir, recentre=False):
    """the arrays of `<split>_sparse_points.npz` (see the module's text), or None without points3D.txt"""
    model_dir = Path(model_dir)
    if not (model_dir / "points3D.txt").exists():
        return None
    cam_id, width, height = read_camera(model_dir / "cameras.txt")[:3]
    images = read_images(model_dir / "images.txt", cam_id)
    points, errors = read_points(model_dir / "points3D.txt"), read_point_errors(model_dir / "points3D.txt")
    shift = CI.optical_axes_meeting_point([im[1] for im in images], [im[2] for im in images]) if recentre else np.zeros(3)
    names, offsets, xy, xyz, error = [], [0], [], [], []
    for name, R, centre, _, obs in images:
        for x, y, pid in obs:
            if pid not in points or not (0.0 <= x < width and 0.0 <= y < height):
                continue
            if (points[pid] - centre) @ -R[:, 2] <= 0.0:      # behind the camera
                continue
            xy.append((x, y))
            xyz.append(points[pid] - shift)
            error.append(errors[pid])
        names.append(name)
        offsets.append(len(xy))
    return dict(names=np.array(names), offsets=np.array(offsets, np.int64), xy=np.array(xy, np.float32).reshape(-1, 2),
                xyz=np.array(xyz, np.float32).reshape(-1, 3), error=np.array(error, np.float32))


def convert(model_dir, near=None, far=None, recentre=False):
    model_dir = Path(model_dir)
    cam_id, width, height, fx, fy, cx, cy, dist = read_camera(model_dir / "cameras.txt")
    images = read_images(model_dir / "images.txt", cam_id)
    if not images:
        raise ValueError(f"{model_dir / 'images.txt'} lists no image")
    points = read_points(model_dir / "points3D.txt") if (model_dir / "points3D.txt").exists() else None
    if points is None and (near is None or far is None):
        raise ValueError("no points3D.txt: give --near and --far")
    shift = CI.optical_axes_meeting_point([im[1] for im in images], [im[2] for im in images]) if recentre else np.zeros(3)
    entries = {}
    for name, R, centre, ids, _ in images:
        if points is not None:
            seen = np.array([points[i] for i in ids if i in points] or list(points.values()))
            lo, hi = CI.depth_bounds(R, centre, seen)
        else:
            lo, hi = near, far
        entries[name] = CI.entry(height, width, fx, fy, cx, cy, dist, R, centre - shift, lo, hi)
    return entries


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-m", "--model_path", required=True, help="directory with cameras.txt, images.txt (and points3D.txt)")
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--near", type=float, default=None)
    ap.add_argument("--far", type=float, default=None)
    ap.add_argument("--recentre", action="store_true")
    ap.add_argument("--no_sparse_points", action="store_true", help="do not write <split>_sparse_points.npz")
    args = ap.parse_args(argv)
    try:
        entries = convert(args.model_path, args.near, args.far, args.recentre)
        sparse = None if args.no_sparse_points else sparse_points(args.model_path, args.recentre)
    except UnsupportedModel as e:
        print(f"convert_from_colmap_text: unsupported: {e}", file=sys.stderr)
        return 2
    path = CI.write_params(args.output_path, args.split, entries)
    print(f"{len(entries)} cameras -> {path}")
    if sparse is not None:
        side = path.with_name(f"{args.split}_sparse_points.npz")
        np.savez(side, **sparse)
        print(f"{len(sparse['xy'])} observations of sparse points -> {side}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
