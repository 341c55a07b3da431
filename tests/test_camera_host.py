"""Host checks of the real-capture camera model: the reference arithmetic tests/camera_ref.py against itself,
PinholeCamera, the dataset schema, the two importers and the C ABI's declarations and validation (no device work)."""
import ctypes
import importlib.util
import io
import json
import os
import pickle
import re

import numpy as np
import pytest
import torch

import camera_ref as CR
from conftest import ROOT
from voxe_hip import abi

K = 3


# ---- the reference arithmetic ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [CR.CAM_C, CR.CAM_D, CR.CAM_B._replace(dist=(0.08, 0.01, -0.001, 0.002, 0.003))])
def test_undistort_inverts_distort(cam):
    xd, yd = np.meshgrid(np.linspace(-1.0, 1.0, 41), np.linspace(-0.75, 0.75, 31))
    xu, yu = CR.undistort(xd, yd, cam.dist)
    dx, dy = CR.distort(xu, yu, cam.dist)
    assert np.abs(dx - xd).max() <= 1e-12 and np.abs(dy - yd).max() <= 1e-12
    x5, y5 = CR.undistort(xd, yd, cam.dist, steps=5)                         # float64 converges in 5 steps
    assert max(np.abs(x5 - xu).max(), np.abs(y5 - yu).max()) <= 1e-12
    # the kernel's float32 6-step iteration over the same extent.  Bound: the residual D(xu) - xd is evaluated to about 3 ulp of
    # |xd| <= 1 (3 x 1.19e-7) and the step divides it by det J >= 0.44 on this extent: 8.1e-7.  Measured: 1.2e-7 .. 3.0e-7
    x32, y32 = CR.undistort(xd, yd, cam.dist, CR.NEWTON_STEPS, np.float32)
    err = max(np.abs(x32 - xu).max(), np.abs(y32 - yu).max())
    print(f"float32 6-step iteration against float64: {err:.2e}")
    assert x32.dtype == np.float32 and err <= 3 * 1.19e-7 / 0.44


def test_jacobian_matches_central_differences():
    rng = np.random.default_rng(0)
    xu, yu = rng.uniform(-0.8, 0.8, 50), rng.uniform(-0.6, 0.6, 50)
    h = 1e-6
    _, _, j00, j01, j11, _ = CR.lens(xu, yu, CR.CAM_D.dist)
    fx = [(a - b) / (2 * h) for a, b in zip(CR.distort(xu + h, yu, CR.CAM_D.dist), CR.distort(xu - h, yu, CR.CAM_D.dist))]
    fy = [(a - b) / (2 * h) for a, b in zip(CR.distort(xu, yu + h, CR.CAM_D.dist), CR.distort(xu, yu - h, CR.CAM_D.dist))]
    for got, want in ((j00, fx[0]), (j01, fx[1]), (j01, fy[0]), (j11, fy[1])):
        assert np.abs(got - want).max() <= 1e-8


@pytest.mark.parametrize("cam", [CR.CAM_B, CR.CAM_D])
def test_every_analytic_gradient_matches_central_differences(cam):
    poses = CR.random_poses(K).astype(np.float64)
    idx = CR.indexed_batch(cam, K, n=200)
    rng = np.random.default_rng(5)
    g_o, g_d = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    d_poses, d_intr, d_dist = CR.cast_rays_bwd(cam, poses, idx, g_o, g_d)

    def fd(make, h):
        return (CR.loss(*make(+h), idx, g_o, g_d) - CR.loss(*make(-h), idx, g_o, g_d)) / (2 * h)

    for j, name in enumerate(("fx", "fy", "cx", "cy")):
        want = fd(lambda h: (cam._replace(**{name: getattr(cam, name) + h}), poses), 1e-5)
        assert abs(d_intr[j] - want) <= 1e-7 * max(abs(want), 1.0), name
    for j in range(5):
        def make(h, j=j):
            dist = list(cam.dist)
            dist[j] += h
            return cam._replace(dist=tuple(dist)), poses
        want = fd(make, 1e-6)
        if cam.distorted:
            assert abs(d_dist[j] - want) <= 1e-6 * max(abs(want), 1.0), j
    for k, a, b in ((0, 0, 0), (1, 2, 1), (2, 1, 3), (0, 2, 3)):
        def make(h, k=k, a=a, b=b):
            p = poses.copy()
            p[k, a, b] += h
            return cam, p
        want = fd(make, 1e-6)
        assert abs(d_poses[k, a, b] - want) <= 1e-7 * max(abs(want), 1.0)


def test_the_stated_bounds_of_the_gpu_tests_hold_for_the_restatement():
    """re-measures what tests/test_camera_gpu.py states: the float32 restatement against float64 on the GPU tests' inputs"""
    G = CR

    poses, idx = CR.random_poses(K), CR.indexed_batch(CR.CAM_C, K)
    worst_fwd = worst_bwd = 0.0
    for cam in (CR.CAM_A, CR.CAM_B, CR.CAM_C, CR.CAM_D):
        for index in (None, idx):
            d64 = CR.cast_rays(cam, poses, index)[1]
            d32 = CR.cast_rays(cam, poses, index, np.float32)[1]
            if cam.distorted:
                worst_fwd = max(worst_fwd, float(np.abs(d32 - d64).max()))
            g_o, g_d = G.upstream(d64.shape[0])
            w = CR.cast_rays_bwd(cam, poses, index, g_o, g_d)
            y = CR.cast_rays_bwd(cam, poses, index, g_o, g_d, np.float32)
            assert G.rel_l2(y[0], w[0]) <= G.POSE_GRAD_REL_L2 / 4
            for a, b in zip(np.concatenate(y[1:]), np.concatenate(w[1:])):
                if b != 0.0:
                    worst_bwd = max(worst_bwd, abs(a - b) / abs(b))
    print(f"float32 restatement against float64: forward {worst_fwd:.3e}, lens gradients {worst_bwd:.3e}")
    assert worst_fwd <= G.FWD_RESTATEMENT_ERR and worst_bwd <= G.LENS_GRAD_RESTATEMENT_ERR
    assert worst_fwd >= 0.5 * G.FWD_RESTATEMENT_ERR and worst_bwd >= 0.5 * G.LENS_GRAD_RESTATEMENT_ERR     # stated, not padded


# ---- PinholeCamera -----------------------------------------------------------------------------------------------------
def _pinhole(cam: CR.Camera):
    from thre3d_atom.utils.imaging_utils import PinholeCamera

    return PinholeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.dist)


def test_pinhole_camera():
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, PinholeCamera, novel_view_camera, scale_camera_intrinsics

    c = _pinhole(CR.CAM_C)
    height, width, focal = c                                                  # unpacks to 3 values, focal = fx
    assert (height, width, focal) == (36, 48, 52.0) and len(c) == 3 and isinstance(c, CameraIntrinsics)
    assert (c.height, c.width, c.focal, c.fx, c.fy, c.cx, c.cy) == (36, 48, 52.0, 52.0, 47.5, 22.3, 19.1)
    assert c.distortion == (-0.12, 0.03, 0.002, -0.001, 0.0)
    back = pickle.loads(pickle.dumps(c))
    assert type(back) is PinholeCamera and back == c and back.distortion == c.distortion and back.cy == 19.1
    buf = io.BytesIO()
    torch.save({"camera_intrinsics": c}, buf)
    buf.seek(0)
    loaded = torch.load(buf, weights_only=False)["camera_intrinsics"]
    assert type(loaded) is PinholeCamera and loaded == c
    assert c != _pinhole(CR.CAM_D) and c != CameraIntrinsics(36, 48, 52.0)      # the model takes part in equality
    # legacy: what (height, width, focal) describes
    legacy = PinholeCamera(800, 800, 1111.111)
    assert legacy.is_legacy() and legacy == CameraIntrinsics(800, 800, 1111.111) and (legacy.cx, legacy.cy, legacy.fy) == (400.0, 400.0, 1111.111)
    assert not c.is_legacy() and not _pinhole(CR.CAM_B).is_legacy() and not PinholeCamera(8, 8, 5.0, 5.0, 4.0, 4.5).is_legacy()
    assert not PinholeCamera(8, 8, 5.0, distortion=(0.01,)).is_legacy()
    # scaled: like the legacy downsampling, 800 px / 3.0 -> 266 px
    s = PinholeCamera(800, 800, 1111.0, 1100.0, 410.0, 395.0, (0.1, 0, 0, 0, 0)).scaled(3.0)
    assert (s.height, s.width) == (266, 266) and s.distortion == (0.1, 0.0, 0.0, 0.0, 0.0)
    assert (s.fx, s.fy, s.cx, s.cy) == (1111.0 / 3.0, 1100.0 / 3.0, 410.0 / 3.0, 395.0 / 3.0)
    u = c.undistorted()
    assert (u.fx, u.fy, u.cx, u.cy, u.distortion) == (c.fx, c.fy, c.cx, c.cy, (0.0,) * 5) and novel_view_camera(c) == u
    plain = CameraIntrinsics(10, 12, 9.0)
    assert novel_view_camera(plain) is plain
    # scale_camera_intrinsics: the subclass keeps its model, a plain tuple behaves as ever
    half = scale_camera_intrinsics(c, 0.5)
    assert type(half) is PinholeCamera and (half.height, half.width, half.fx, half.cy) == (18, 24, 26.0, 9.55) and half.distortion == c.distortion
    assert type(scale_camera_intrinsics(plain, 0.5)) is CameraIntrinsics and scale_camera_intrinsics(plain, 0.5) == CameraIntrinsics(5, 6, 4.5)


def test_validate_accepts_the_test_cameras_and_rejects_the_strong_barrel():
    for cam in (CR.CAM_B, CR.CAM_C, CR.CAM_D):
        assert _pinhole(cam).validate() is not None
    with pytest.raises(ValueError, match="not invertible"):
        _pinhole(CR.STRONG_BARREL).validate()
    with pytest.raises(ValueError):
        _pinhole(CR.CAM_B._replace(fx=0.0)).validate()
    with pytest.raises(ValueError):
        _pinhole(CR.CAM_C._replace(dist=(float("nan"), 0, 0, 0, 0))).validate()


# ---- the dataset schema ------------------------------------------------------------------------------------------------
def _write_dataset(tmp_path, intrinsic_of, n=3, hw=(6, 8)):
    from PIL import Image

    (tmp_path / "train").mkdir(parents=True, exist_ok=True)
    poses = CR.random_poses(n)
    params = {}
    for i in range(n):
        name = f"{i:04d}.png"
        Image.fromarray(np.full((*hw, 3), 40 * i, np.uint8)).save(tmp_path / "train" / name)
        params[name] = {"intrinsic": {"height": hw[0], "width": hw[1], "bounds": [1.0, 4.0], **intrinsic_of(i)},
                        "extrinsic": {"rotation": poses[i, :, :3].tolist(), "translation": poses[i, :, 3:].tolist()}}
    (tmp_path / "train_camera_params.json").write_text(json.dumps(params))
    return tmp_path / "train", tmp_path / "train_camera_params.json"


def test_dataset_reads_the_camera_model(tmp_path):
    from thre3d_atom.data.datasets import PosedImagesDataset
    from thre3d_atom.thre3d_reprs.poses import write_camera_params
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, PinholeCamera

    legacy = PosedImagesDataset(*_write_dataset(tmp_path / "legacy", lambda i: {"focal": 11.5}))
    assert type(legacy.camera_intrinsics) is CameraIntrinsics and legacy.camera_intrinsics == CameraIntrinsics(6, 8, 11.5)
    model = {"focal": 11.5, "fx": 11.5, "fy": 10.5, "cx": 4.2, "cy": 2.9, "distortion": [-0.05, 0.01, 0.001, 0.0, 0.0]}
    data = PosedImagesDataset(*_write_dataset(tmp_path / "model", lambda i: model))
    want = PinholeCamera(6, 8, 11.5, 10.5, 4.2, 2.9, (-0.05, 0.01, 0.001, 0.0, 0.0))
    assert type(data.camera_intrinsics) is PinholeCamera and data.camera_intrinsics == want
    # downsampled() carries the model
    half = data.downsampled(2.0)
    assert half.camera_intrinsics == want.scaled(2.0) and half.images.shape[-2:] == (3, 4)
    assert type(legacy.downsampled(2.0).camera_intrinsics) is CameraIntrinsics
    # write_camera_params keeps it, and can replace it
    path = write_camera_params(tmp_path / "out.json", data, data.poses)
    assert PosedImagesDataset(tmp_path / "model" / "train", path).camera_intrinsics == want
    moved = want.with_intrinsics(12.0, 11.0, 4.0, 3.0)
    path = write_camera_params(tmp_path / "out2.json", data, data.poses, camera=moved)
    assert PosedImagesDataset(tmp_path / "model" / "train", path).camera_intrinsics == moved
    # entries that disagree: one shared camera per dataset
    with pytest.raises(ValueError, match="one shared camera"):
        PosedImagesDataset(*_write_dataset(tmp_path / "mixed", lambda i: dict(model, fy=10.5 + i)))
    with pytest.raises(ValueError, match="one shared camera"):
        PosedImagesDataset(*_write_dataset(tmp_path / "partial", lambda i: model if i else {"focal": 11.5}))
    # a lens model outside its monotonic region does not load
    with pytest.raises(ValueError, match="not invertible"):
        PosedImagesDataset(*_write_dataset(tmp_path / "barrel", lambda i: {"fx": 4.4, "fy": 4.3, "distortion": [-0.5, 0.0, 0.0, 0.0, 0.0]}))


# ---- the importers -----------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _matrix_to_quaternion(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-6:
        return np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)])


def _look_at(eye, target=(0.0, 0.0, 0.0)):
    """world-to-camera (R, t) in COLMAP's / OpenCV's axes: x right, y DOWN, looking down +z"""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ eye


def _opencv_pixel(R, t, fx, fy, cx, cy, dist, point):
    """the pixel OpenCV's own projection puts `point` at: written in COLMAP's convention, independent of camera_ref"""
    k1, k2, p1, p2, k3 = dist
    pc = R @ np.asarray(point, np.float64) + t
    x, y = pc[0] / pc[2], pc[1] / pc[2]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    return (fx * (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx, fy * (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy)


EYES = ((3.0, 0.5, 1.0), (-1.0, 3.0, 1.5), (0.5, -3.0, 2.0))
POINT = (0.2, -0.15, 0.1)
CLOUD = np.random.default_rng(4).uniform(-0.5, 0.5, size=(40, 3))
COLMAP_MODELS = {
    "SIMPLE_PINHOLE": ("60 31.5 24.5", (60, 60, 31.5, 24.5, (0, 0, 0, 0, 0))),
    "PINHOLE": ("60 57 31.5 24.5", (60, 57, 31.5, 24.5, (0, 0, 0, 0, 0))),
    "SIMPLE_RADIAL": ("60 31.5 24.5 -0.08", (60, 60, 31.5, 24.5, (-0.08, 0, 0, 0, 0))),
    "RADIAL": ("60 31.5 24.5 -0.08 0.02", (60, 60, 31.5, 24.5, (-0.08, 0.02, 0, 0, 0))),
    "OPENCV": ("60 57 31.5 24.5 -0.08 0.02 0.002 -0.001", (60, 57, 31.5, 24.5, (-0.08, 0.02, 0.002, -0.001, 0))),
}


def _write_colmap(path, model, cameras=1, points=True):
    path.mkdir(parents=True, exist_ok=True)
    text = "# Camera list with one line of data per camera:\n" + "".join(
        f"{i + 1} {model} 64 48 {COLMAP_MODELS[model][0]}\n" for i in range(cameras))
    (path / "cameras.txt").write_text(text)
    lines = ["# Image list with two lines of data per image:"]
    for i, eye in enumerate(EYES):
        R, t = _look_at(eye)
        q = _matrix_to_quaternion(R)
        lines.append(f"{i + 1} {' '.join(repr(float(v)) for v in q)} {' '.join(repr(float(v)) for v in t)} 1 img_{i}.png")
        lines.append(" ".join(f"10.0 10.0 {j + 1}" for j in range(len(CLOUD))) if points else "")
    (path / "images.txt").write_text("\n".join(lines) + "\n")
    if points:
        (path / "points3D.txt").write_text("# 3D point list\n" + "".join(
            f"{j + 1} {p[0]!r} {p[1]!r} {p[2]!r} 128 128 128 0.5 1 0\n" for j, p in enumerate(CLOUD.tolist())))


def _check_projection(entries, names, fx, fy, cx, cy, dist):
    assert list(entries) == names
    for name, eye in zip(names, EYES):
        e = entries[name]
        i = e["intrinsic"]
        cam = CR.Camera(i["height"], i["width"], i["fx"], i["fy"], i["cx"], i["cy"], tuple(i["distortion"]))
        assert (cam.H, cam.W, i["focal"]) == (48, 64, i["fx"])
        pose = np.concatenate([np.array(e["extrinsic"]["rotation"]), np.array(e["extrinsic"]["translation"])], axis=1)
        assert np.allclose(pose[:, 3], eye, atol=1e-12) and np.allclose(pose[:, :3].T @ pose[:, :3], np.eye(3), atol=1e-12)
        assert np.linalg.det(pose[:, :3]) > 0.999
        want = _opencv_pixel(*_look_at(eye), fx, fy, cx, cy, dist, POINT)
        got = CR.project(cam, pose, POINT)
        assert 0 < want[0] < 64 and 0 < want[1] < 48                                      # the point is in the image
        assert abs(got[0] - want[0]) <= 1e-9 and abs(got[1] - want[1]) <= 1e-9, (name, got, want)
        # and the ray cast through that pixel's position passes through the point: the axis conventions of the caster
        xu, yu = CR.undistort((want[0] - cam.cx) / cam.fx, (want[1] - cam.cy) / cam.fy, cam.dist)
        ray = pose[:, :3] @ np.array([xu, -yu, -1.0])
        to_point = np.asarray(POINT) - pose[:, 3]
        assert np.linalg.norm(np.cross(ray, to_point)) <= 1e-9 * np.linalg.norm(ray) * np.linalg.norm(to_point) and ray @ to_point > 0


@pytest.mark.parametrize("model", list(COLMAP_MODELS))
def test_colmap_importer(tmp_path, model):
    from thre3d_atom.data.datasets import camera_from_params

    tool = _tool("convert_from_colmap_text")
    _write_colmap(tmp_path / "sparse", model)
    assert tool.main(["-m", str(tmp_path / "sparse"), "-o", str(tmp_path / "scene")]) == 0
    entries = json.loads((tmp_path / "scene" / "train_camera_params.json").read_text())
    fx, fy, cx, cy, dist = COLMAP_MODELS[model][1]
    _check_projection(entries, [f"img_{i}.png" for i in range(3)], fx, fy, cx, cy, dist)
    cam = camera_from_params(entries, "img_0.png")                          # the dataset reads what the tool wrote
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.distortion) == (fx, fy, cx, cy, tuple(float(v) for v in dist))
    # bounds from the point cloud: 1st / 99th percentile of the depths along the view direction
    for i, eye in enumerate(EYES):
        R, t = _look_at(eye)
        depth = (CLOUD @ R.T + t)[:, 2]
        near, far = entries[f"img_{i}.png"]["intrinsic"]["bounds"]
        assert abs(near - np.percentile(depth, 1)) <= 1e-9 and abs(far - np.percentile(depth, 99)) <= 1e-9
    # --recentre: these cameras all look at the origin, so nothing moves
    assert tool.main(["-m", str(tmp_path / "sparse"), "-o", str(tmp_path / "centred"), "--recentre"]) == 0
    centred = json.loads((tmp_path / "centred" / "train_camera_params.json").read_text())
    for name in entries:
        assert np.allclose(centred[name]["extrinsic"]["translation"], entries[name]["extrinsic"]["translation"], atol=1e-9)


def test_colmap_importer_bounds_options_and_refusals(tmp_path, capsys):
    tool = _tool("convert_from_colmap_text")
    _write_colmap(tmp_path / "nopoints", "OPENCV", points=False)
    with pytest.raises(ValueError, match="--near and --far"):
        tool.convert(tmp_path / "nopoints")
    entries = tool.convert(tmp_path / "nopoints", near=0.5, far=6.0)
    assert all(e["intrinsic"]["bounds"] == [0.5, 6.0] for e in entries.values())
    _write_colmap(tmp_path / "two", "PINHOLE", cameras=2)
    assert tool.main(["-m", str(tmp_path / "two"), "-o", str(tmp_path / "out")]) == 2
    err = capsys.readouterr().err
    assert "holds 2 cameras" in err and "exactly one shared camera" in err and not (tmp_path / "out").exists()
    (tmp_path / "two" / "cameras.txt").write_text("1 OPENCV_FISHEYE 64 48 60 57 31.5 24.5 0 0 0 0\n")
    with pytest.raises(tool.UnsupportedModel, match="OPENCV_FISHEYE is not supported"):
        tool.convert(tmp_path / "two")


def test_recentre_moves_the_meeting_point_of_the_optical_axes_to_the_origin():
    CI = _tool("camera_import")
    target = np.array([0.7, -0.4, 0.3])
    rots, centres = [], []
    for eye in EYES:
        R, t = _look_at(eye, target)
        rots.append(R.T @ np.diag([1.0, -1.0, -1.0]))
        centres.append(-R.T @ t)
    assert np.allclose(CI.optical_axes_meeting_point(rots, centres), target, atol=1e-12)


def test_nerfstudio_importer(tmp_path, capsys):
    tool = _tool("convert_from_nerfstudio_transforms")
    fx, fy, cx, cy, dist = 60.0, 57.0, 31.5, 24.5, (-0.08, 0.02, 0.002, -0.001, 0.0)
    frames = []
    for i, eye in enumerate(EYES):
        R, t = _look_at(eye)
        c2w = np.eye(4)
        c2w[:3, :3] = R.T @ np.diag([1.0, -1.0, -1.0])                        # OpenGL camera-to-world
        c2w[:3, 3] = -R.T @ t
        frames.append({"file_path": f"images/img_{i}.png", "transform_matrix": c2w.tolist()})
    meta = {"w": 64, "h": 48, "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy, "k1": dist[0], "k2": dist[1], "p1": dist[2], "p2": dist[3],
            "camera_model": "OPENCV", "frames": frames}
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    assert tool.main(["-t", str(tmp_path / "transforms.json"), "-o", str(tmp_path / "scene"), "--near", "0.5", "--far", "6"]) == 0
    entries = json.loads((tmp_path / "scene" / "train_camera_params.json").read_text())
    _check_projection(entries, [f"img_{i}.png" for i in range(3)], fx, fy, cx, cy, dist)
    assert all(e["intrinsic"]["bounds"] == [0.5, 6.0] for e in entries.values())
    frames[1]["fl_x"] = 61.0
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    assert tool.main(["-t", str(tmp_path / "transforms.json"), "-o", str(tmp_path / "bad"), "--near", "0.5", "--far", "6"]) == 2
    assert "per-frame intrinsics are not supported" in capsys.readouterr().err
    meta["camera_model"] = "OPENCV_FISHEYE"
    (tmp_path / "transforms.json").write_text(json.dumps(meta))
    with pytest.raises(tool.UnsupportedModel, match="fisheye"):
        tool.convert(tmp_path / "transforms.json", 0.5, 6.0)


# ---- the C ABI: declarations and validation without a device -----------------------------------------------------------
def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_symbols_struct_and_abi_version():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    for name in ("voxe_cast_rays_camera", "voxe_cast_rays_camera_bwd_scratch_bytes", "voxe_cast_rays_camera_bwd"):
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name)
    assert not re.search(r"\bvoxe_cpu_cast_rays_camera", text)
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text and L.voxe_abi_version() == 13
    assert "voxe_camera.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    assert ctypes.sizeof(abi.VoxeCamera) == 44 and [f[0] for f in abi.VoxeCamera._fields_] == ["H", "W", "fx", "fy", "cx", "cy", "k1", "k2",
                                                                                                 "p1", "p2", "k3"]
    assert "NOT promised bit-reproducible" in text[text.index("voxe_cast_rays_camera_bwd:"):]


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)
    need = L.voxe_cast_rays_camera_bwd_scratch_bytes(3)
    assert need >= (3 * 12 + 9) * 8

    def cam(**kw):
        c = abi.VoxeCamera(4, 5, 3.0, 3.5, 2.4, 2.1, -0.1, 0.02, 0.001, -0.001, 0.003)
        for k, v in kw.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    def fwd(c=None, poses=P, K=3, idx=P, B=7, o=P, d=P):
        return L.voxe_cast_rays_camera(None if c == "null" else c or cam(), poses, K, idx, B, o, d, None)

    def bwd(c=None, poses=P, K=3, idx=P, B=7, d_poses=P, d_i=P, d_k=P, sc=P, nbytes=need):
        return L.voxe_cast_rays_camera_bwd(None if c == "null" else c or cam(), poses, K, idx, B, P, P, d_poses, d_i, d_k, 0, sc, nbytes, None)

    for call in (fwd, bwd):
        for bad in (dict(H=0), dict(W=-1), dict(fx=0.0), dict(fy=-2.0), dict(fx=float("inf")), dict(fy=float("nan")),
                    dict(cx=float("nan")), dict(cy=float("inf")), dict(k1=float("nan")), dict(k2=float("inf")), dict(p1=float("nan")),
                    dict(p2=float("nan")), dict(k3=float("-inf"))):
            assert call(c=cam(**bad)) == abi.ERR_BAD_SHAPE, bad
        assert call(K=0) == abi.ERR_BAD_SHAPE and call(B=-1) == abi.ERR_BAD_SHAPE
        assert call(idx=None, B=59) == abi.ERR_BAD_SHAPE                                  # whole images: B == K H W
        assert call(poses=None) == abi.ERR_NULL_POINTER and call(c="null") == abi.ERR_NULL_POINTER
    assert fwd(o=None) == abi.ERR_NULL_POINTER and fwd(d=None) == abi.ERR_NULL_POINTER
    assert fwd(B=0) == abi.OK and fwd(B=0, o=None, d=None) == abi.OK                      # no launch, nothing written
    assert bwd(sc=None) == abi.ERR_WORKSPACE and bwd(nbytes=need - 1) == abi.ERR_WORKSPACE
    assert bwd(d_poses=None, d_i=None, d_k=None, sc=None) == abi.OK                       # all outputs NULL: no launch
    assert bwd(B=0, d_poses=None, d_i=None, d_k=None) == abi.OK


def test_operators_refuse_host_tensors():
    from voxe_hip import ops
    from voxe_hip.runtime import VoxeError

    for call in (lambda: ops.cast_rays_camera((4, 4, 5.0), torch.zeros(1, 3, 4)),
                 lambda: ops.cast_rays_camera_bwd((4, 4, 5.0), torch.zeros(1, 3, 4), None, None, None),
                 lambda: ops.cast_rays_from_camera((4, 4, 5.0), torch.zeros(1, 3, 4))):
        with pytest.raises(VoxeError):
            call()


def test_the_recorded_float64_recovery_ratio():
    """the float64 run of the intrinsics-recovery problem, whose ratio tests/test_camera_gpu.py holds the GPU run to"""
    ratio, losses = CR.recovery_float64()
    print(f"float64 intrinsics recovery: |error| ratio {ratio:.5f}; loss {losses[0]:.3e} -> {losses[-1]:.3e}")
    assert abs(ratio - CR.RECOVERY_RATIO_FLOAT64) <= 0.02 * CR.RECOVERY_RATIO_FLOAT64 and losses[-1] < 1e-3 * losses[0]
