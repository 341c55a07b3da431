"""Reference arithmetic of the real-capture camera model (include/voxe.h, voxe_cast_rays_camera).

numpy float64 with Newton run to convergence (the truth the kernels are held to), the chain rule by the implicit-function
theorem, a projection (world point -> pixel), and a float32 restatement of the kernel's own arithmetic: its exact 6-step
iteration and its float32-per-ray / double-sum backward.  numpy float32 scalars round every operation, like the kernels built
without FMA.  A camera here is (H, W, fx, fy, cx, cy, (k1, k2, p1, p2, k3)): `Camera`."""
from typing import NamedTuple, Tuple

import numpy as np

NEWTON_STEPS = 6          # the kernel's


class Camera(NamedTuple):
    H: int
    W: int
    fx: float
    fy: float
    cx: float
    cy: float
    dist: Tuple[float, float, float, float, float] = (0.0, 0.0, 0.0, 0.0, 0.0)

    @property
    def distorted(self):
        return any(v != 0.0 for v in self.dist)


# the cameras of tests/test_camera_gpu.py (H = 36, W = 48: a wave straddles image rows)
H, W = 36, 48
LEGACY_FOCAL = 55.0
CAM_A = Camera(H, W, LEGACY_FOCAL, LEGACY_FOCAL, W * 0.5, H * 0.5)
CAM_B = Camera(H, W, 52.0, 47.5, 22.3, 19.1)
CAM_C = CAM_B._replace(dist=(-0.12, 0.03, 0.002, -0.001, 0.0))
CAM_D = CAM_B._replace(dist=(-0.20, 0.05, 0.0015, -0.001, -0.004))
# outside the monotonic region at its field of view (0.9 x 0.7): PinholeCamera.validate() must reject it; never cast
STRONG_BARREL = Camera(H, W, (W * 0.5) / 0.9, (H * 0.5) / 0.7, W * 0.5, H * 0.5, (-0.28, 0.09, 0.001, 0.0015, -0.012))


def lens(xu, yu, dist, dtype=np.float64):
    """D(xu, yu) and the entries of its symmetric Jacobian (j00, j01, j11), r2 -- the kernel's expressions, in `dtype`"""
    k1, k2, p1, p2, k3 = (dtype(v) for v in dist)
    one, two, three, six = dtype(1), dtype(2), dtype(3), dtype(6)
    xx, yy, xy = xu * xu, yu * yu, xu * yu
    r2 = xx + yy
    rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (two * k2 + three * r2 * k3)
    dx = xu * rad + two * p1 * xy + p2 * (r2 + two * xx)
    dy = yu * rad + p1 * (r2 + two * yy) + two * p2 * xy
    j00 = rad + two * xx * drad + two * p1 * yu + six * p2 * xu
    j01 = two * xy * drad + two * p1 * xu + two * p2 * yu
    j11 = rad + two * yy * drad + six * p1 * yu + two * p2 * xu
    return dx, dy, j00, j01, j11, r2


def distort(xu, yu, dist):
    dx, dy, *_ = lens(np.asarray(xu, np.float64), np.asarray(yu, np.float64), dist)
    return dx, dy


def undistort(xd, yd, dist, steps=50, dtype=np.float64):
    """Newton from (xd, yd); float64 / 50 steps: converged (it needs 5); float32 / NEWTON_STEPS: the kernel's iteration"""
    xd, yd = np.asarray(xd, dtype), np.asarray(yd, dtype)
    xu, yu = xd.copy(), yd.copy()
    for _ in range(steps):
        dx, dy, j00, j01, j11, _ = lens(xu, yu, dist, dtype)
        ex, ey = dx - xd, dy - yd
        det = j00 * j11 - j01 * j01
        xu, yu = xu - (j11 * ex - j01 * ey) / det, yu - (j00 * ey - j01 * ex) / det
    return xu, yu


def decode(cam: Camera, K, flat_index):
    per = cam.H * cam.W
    f = np.arange(K * per, dtype=np.int64) if flat_index is None else np.asarray(flat_index, np.int64)
    k = np.clip(f // per, 0, K - 1)
    rem = f - (f // per) * per
    return k, rem % cam.W, rem // cam.W


def normalised(cam: Camera, px, py, dtype=np.float64):
    """(xd, yd, xu, yu) of pixels; float32: the kernel's arithmetic and iteration"""
    half = dtype(0.5)
    xd = (px.astype(dtype) + half - dtype(cam.cx)) / dtype(cam.fx)
    yd = (py.astype(dtype) + half - dtype(cam.cy)) / dtype(cam.fy)
    if not cam.distorted:
        return xd, yd, xd, yd
    xu, yu = undistort(xd, yd, cam.dist, 50 if dtype is np.float64 else NEWTON_STEPS, dtype)
    return xd, yd, xu, yu


def cast_rays(cam: Camera, poses, flat_index=None, dtype=np.float64):
    """rays_o, rays_d [B,3] of poses [K,3,4]"""
    poses = np.asarray(poses, dtype)
    k, px, py = decode(cam, poses.shape[0], flat_index)
    _, _, xu, yu = normalised(cam, px, py, dtype)
    R = poses[k]
    dz = dtype(-1.0)
    d = np.stack([(R[:, r, 0] * xu + R[:, r, 1] * (-yu)) + R[:, r, 2] * dz for r in range(3)], axis=1)
    return R[:, :, 3].copy(), d


def cast_rays_bwd(cam: Camera, poses, flat_index, g_o, g_d, per_ray=np.float64):
    """(d_poses [K,3,4], d_intrinsics [4] fx fy cx cy, d_distortion [5] k1 k2 p1 p2 k3), float64 sums.  per_ray float32: the
    kernel's per-ray arithmetic (its 6-step forward, float32 terms of the intrinsics and coefficients)."""
    t = per_ray
    poses64 = np.asarray(poses, np.float64)
    K = poses64.shape[0]
    k, px, py = decode(cam, K, flat_index)
    xd, yd, xu, yu = normalised(cam, px, py, t)
    B = k.shape[0]
    g_o = np.zeros((B, 3)) if g_o is None else np.asarray(g_o, np.float64)
    g_d = np.zeros((B, 3), t) if g_d is None else np.asarray(g_d, t)
    dc = np.stack([xu, -yu, np.full_like(xu, -1.0)], axis=1)
    d_poses = np.zeros((K, 3, 4))
    np.add.at(d_poses[:, :, :3], k, g_d.astype(np.float64)[:, :, None] * dc.astype(np.float64)[:, None, :])
    np.add.at(d_poses[:, :, 3], k, g_o)
    R = np.asarray(poses, t)[k]
    g_xu = (R[:, 0, 0] * g_d[:, 0] + R[:, 1, 0] * g_d[:, 1]) + R[:, 2, 0] * g_d[:, 2]
    g_yu = -((R[:, 0, 1] * g_d[:, 0] + R[:, 1, 1] * g_d[:, 1]) + R[:, 2, 1] * g_d[:, 2])
    w = np.zeros((9, B), t)
    g_xd, g_yd = g_xu, g_yu
    if cam.distorted:
        _, _, j00, j01, j11, r2 = lens(xu, yu, cam.dist, t)
        det = j00 * j11 - j01 * j01
        g_xd = (j11 * g_xu - j01 * g_yu) / det
        g_yd = (j00 * g_yu - j01 * g_xu) / det
        two = t(2)
        xx, yy, xy = xu * xu, yu * yu, xu * yu
        radial = g_xd * xu + g_yd * yu
        w[4] = -(radial * r2)
        w[5] = -(radial * (r2 * r2))
        w[8] = -(radial * ((r2 * r2) * r2))
        w[6] = -(g_xd * (two * xy) + g_yd * (r2 + two * yy))
        w[7] = -(g_xd * (r2 + two * xx) + g_yd * (two * xy))
    w[0] = -(g_xd * xd) / t(cam.fx)
    w[1] = -(g_yd * yd) / t(cam.fy)
    w[2] = -g_xd / t(cam.fx)
    w[3] = -g_yd / t(cam.fy)
    sums = w.astype(np.float64).sum(axis=1)
    return d_poses, sums[:4], sums[4:]


def loss(cam: Camera, poses, flat_index, g_o, g_d):
    """the scalar whose gradient cast_rays_bwd is"""
    o, d = cast_rays(cam, poses, flat_index)
    return float((o * g_o).sum() + (d * g_d).sum())


def project(cam: Camera, pose, point):
    """pixel coordinates (continuous; pixel (px, py) covers [px, px+1) x [py, py+1)) of a world point seen from pose [3,4]
    (camera-to-world, x right, y up, looking down -z), or None when it lies behind the camera"""
    pose = np.asarray(pose, np.float64)
    pc = pose[:, :3].T @ (np.asarray(point, np.float64) - pose[:, 3])
    if pc[2] >= 0:
        return None
    xu, yu = pc[0] / -pc[2], -pc[1] / -pc[2]
    xd, yd = distort(xu, yu, cam.dist)
    return float(xd * cam.fx + cam.cx), float(yd * cam.fy + cam.cy)


def random_poses(K, seed=0, radius=4.0):
    """K random camera-to-world poses [K,3,4] float32 looking roughly at the origin"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(np.concatenate([q, (q[:, 2] * radius + 0.1 * rng.normal(size=3))[:, None]], axis=1))
    return np.stack(out).astype(np.float32)


def indexed_batch(cam: Camera, K, n=1000, seed=1):
    """n shuffled flat indices with duplicates and both corners of the image stack"""
    rng = np.random.default_rng(seed)
    total = K * cam.H * cam.W
    idx = rng.integers(0, total, size=n - 4)
    idx = np.concatenate([idx, [0, total - 1, idx[0], idx[1]]])
    rng.shuffle(idx)
    return idx.astype(np.int64)


# ---- what the GPU tests and the host tests share -------------------------------------------------------------------------
# Bounds of tests/test_camera_gpu.py, measured on the CPU with this module on that file's exact inputs
# (tests/test_camera_host.py re-measures them): the float32 restatement against float64
FWD_RESTATEMENT_ERR = 1.14e-7          # max |rays_d|, cameras (c) 1.10e-7 and (d) 1.14e-7
FWD_BOUND = 4.0 * FWD_RESTATEMENT_ERR
LENS_GRAD_RESTATEMENT_ERR = 1.10e-6    # per component of d_intrinsics / d_distortion, relative to its own magnitude
LENS_GRAD_BOUND = 4.0 * LENS_GRAD_RESTATEMENT_ERR
POSE_GRAD_REL_L2 = 1e-6                # the bound tests/test_ray_grad_gpu.py holds voxe_cast_rays_bwd to


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def upstream(B):
    g = np.random.default_rng(11)
    return g.normal(size=(B, 3)).astype(np.float32), g.normal(size=(B, 3)).astype(np.float32)


# ---- torch float64 restatement, differentiable w.r.t. the intrinsics (tests 5 and 6) -------------------------------------
def cast_rays_torch(cam: Camera, intrinsics, poses, flat_index=None):
    """(rays_o, rays_d) [B,3] float64 of poses [K,3,4] with `intrinsics` = tensor [4] (fx fy cx cy) in place of the camera's own;
    differentiable w.r.t. `intrinsics`.  Newton runs to convergence without a graph; one more step from the converged point
    carries exactly the implicit-function derivative."""
    import torch

    poses = torch.as_tensor(poses, dtype=torch.float64)
    k, px, py = decode(cam, poses.shape[0], None if flat_index is None else np.asarray(flat_index))
    k, x, y = torch.from_numpy(k), torch.from_numpy(px + 0.5), torch.from_numpy(py + 0.5)
    fx, fy, cx, cy = intrinsics.to(torch.float64)
    xd, yd = (x - cx) / fx, (y - cy) / fy
    xu, yu = xd, yd
    if cam.distorted:
        x0, y0 = undistort(xd.detach().numpy(), yd.detach().numpy(), cam.dist)
        x0, y0 = torch.from_numpy(x0), torch.from_numpy(y0)
        dx, dy, j00, j01, j11, _ = lens(x0, y0, cam.dist, lambda v: torch.tensor(float(v), dtype=torch.float64))
        ex, ey = dx - xd, dy - yd
        det = j00 * j11 - j01 * j01
        xu, yu = x0 - (j11 * ex - j01 * ey) / det, y0 - (j00 * ey - j01 * ex) / det
    dirs = torch.stack([xu, -yu, -torch.ones_like(xu)], dim=1)
    R = poses[k]
    return R[:, :, 3], (R[:, :, :3] * dirs[:, None, :]).sum(dim=-1)


# the intrinsics-recovery problem of test 6 (and the scene of test 5): camera (c) at 32 x 24, 4 poses, a 24^3 SH-0 grid
SMALL_H, SMALL_W = 24, 32
CAM_C_SMALL = Camera(SMALL_H, SMALL_W, CAM_C.fx * SMALL_W / W, CAM_C.fy * SMALL_H / H, CAM_C.cx * SMALL_W / W, CAM_C.cy * SMALL_H / H,
                     CAM_C.dist)
RECOVERY_STEPS, RECOVERY_LR, RECOVERY_SEED, RECOVERY_SAMPLES, RECOVERY_DENSITY_SCALE = 100, 0.05, 7, 64, 10.0
# final |intrinsics - truth| / initial |intrinsics - truth| of the float64 run below (recovery_float64(), on the CPU):
# tests/test_camera_host.py re-runs it; the GPU run of tests/test_camera_gpu.py must end within 1.5 x this
RECOVERY_RATIO_FLOAT64 = 0.01416          # loss 1.894e-2 -> 1.643e-6


def recovery_truth():
    c = CAM_C_SMALL
    return np.array([c.fx, c.fy, c.cx, c.cy])


def recovery_start():
    """fx, fy + 3 %, cx, cy + 1.5 px"""
    t = recovery_truth()
    return np.array([t[0] * 1.03, t[1] * 1.03, t[2] + 1.5, t[3] + 1.5])


def recovery_poses():
    import torch
    from thre3d_atom.utils.imaging_utils import pose_spherical
    from voxe_hip import workload

    return torch.stack([torch.cat(pose_spherical(90.0 * i + 20.0, 25.0 + 12.0 * i, workload.RADIUS), dim=1) for i in range(4)])


def recovery_grid():
    """(densities [24,24,24,1], features [24,24,24,3]) of tests/synth.py's sphere scene"""
    import synth

    return synth.sphere_grid(24)


def recovery_float64():
    """the refiner's problem (thre3d_atom/modules/pose_refiner.py: frozen grid, exact poses, per iteration 4 cameras drawn with
    replacement, MSE over all their pixels, Adam on fx fy cx cy) in float64 on the host -> (error ratio, losses)"""
    import torch
    import ray_grad_ref as RR
    import synth
    from voxe_hip import abi, ops

    dens, feat = recovery_grid()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=RECOVERY_DENSITY_SCALE, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    params = ops.RenderParams(num_samples=RECOVERY_SAMPLES, near=synth.NEAR, far=synth.FAR, white_bkgd=True)
    poses = recovery_poses().double()
    cam = CAM_C_SMALL

    def render(intr, p):
        ro, rd = cast_rays_torch(cam, intr, p)
        samples = RR.probe_host(spec, params, dens, feat, ro, rd)
        return RR.render_from_samples(*samples, dens, feat, ro, rd, spec, params)[0]

    truth = torch.from_numpy(recovery_truth())
    with torch.no_grad():
        target = render(truth, poses).reshape(4, -1, 3)
    intr = torch.nn.Parameter(torch.from_numpy(recovery_start()))
    opt = torch.optim.Adam([intr], lr=RECOVERY_LR)
    gen = torch.Generator().manual_seed(RECOVERY_SEED)
    losses = []
    for _ in range(RECOVERY_STEPS):
        picks = torch.randint(0, 4, (4,), generator=gen)
        loss = torch.nn.functional.mse_loss(render(intr, poses[picks]), target[picks].reshape(-1, 3))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    start, end = recovery_start() - recovery_truth(), intr.detach().numpy() - recovery_truth()
    return float(np.linalg.norm(end) / np.linalg.norm(start)), losses
