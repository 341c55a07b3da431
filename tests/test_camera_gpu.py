"""GPU checks of the real-capture camera model (voxe_cast_rays_camera, voxe_cast_rays_camera_bwd, ops.cast_rays_from_camera,
--intrinsics_learning_rate, the trainer's routing) against tests/camera_ref.py.

Shapes: H = 36, W = 48 (non-square: a wave straddles image rows), K = 3 random poses; whole images (B = 5184), an indexed batch
of 1000 shuffled indices with duplicates and both corners, B = 1 and B = 0.  Cameras: camera_ref.CAM_A .. CAM_D.

Bounds, measured on the CPU with tests/camera_ref.py on these exact inputs (tests/test_camera_host.py re-measures them):
  forward, cameras (c) and (d): the float32 restatement of the kernel's 6-step iteration is within 1.14e-7 of float64 in
      max |rays_d| (1.10e-7 for (c), 1.14e-7 for (d)); x 4 for operation order: FWD_BOUND = 4.6e-7.
  backward, d_intrinsics and d_distortion: the float32-per-ray / double-sum restatement is within 1.10e-6 of float64 relative
      to each component's own magnitude (worst: k2 of camera (c), whole images); x 4: LENS_GRAD_BOUND = 4.4e-6 per component.
  d_poses: 1e-6 rel-L2, the bound tests/test_ray_grad_gpu.py holds voxe_cast_rays_bwd to (double sums, cast once)."""
import ctypes

import numpy as np
import pytest
import torch

import camera_ref as CR
from voxe_hip import abi, ops
from voxe_hip.runtime import VoxeError, lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

K = 3
FWD_RESTATEMENT_ERR, FWD_BOUND = CR.FWD_RESTATEMENT_ERR, CR.FWD_BOUND
LENS_GRAD_RESTATEMENT_ERR, LENS_GRAD_BOUND = CR.LENS_GRAD_RESTATEMENT_ERR, CR.LENS_GRAD_BOUND
POSE_GRAD_REL_L2 = CR.POSE_GRAD_REL_L2
rel_l2, upstream = CR.rel_l2, CR.upstream
CAMERAS = {"a": CR.CAM_A, "b": CR.CAM_B, "c": CR.CAM_C, "d": CR.CAM_D}


def struct(cam: CR.Camera) -> abi.VoxeCamera:
    return abi.VoxeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, *cam.dist)


@pytest.fixture(scope="module")
def scene():
    poses = CR.random_poses(K)
    idx = CR.indexed_batch(CR.CAM_C, K)
    assert len(np.unique(idx)) < len(idx) and idx.min() == 0 and idx.max() == K * CR.H * CR.W - 1
    return dict(poses=poses, idx=idx, poses_t=torch.from_numpy(poses).to(DEV), idx_t=torch.from_numpy(idx).to(DEV))


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- 1: the legacy-equivalent camera gives the legacy caster's bits ------------------------------------------------------
def test_legacy_equivalent_camera_is_bit_exact_with_the_legacy_casters(scene):
    cam, poses = struct(CR.CAM_A), scene["poses_t"]
    one = torch.tensor([CR.H * CR.W + 7 * CR.W + 5], device=DEV)
    for idx in (scene["idx_t"], one, torch.arange(K * CR.H * CR.W, device=DEV)):
        o, d = ops.cast_rays_camera(cam, poses, idx)
        lo, ld = ops.cast_rays_indexed(CR.H, CR.W, CR.LEGACY_FOCAL, poses, idx)
        assert torch.equal(o, lo) and np.array_equal(bits(d), bits(ld)) and d.shape == (idx.shape[0], 3)
    o, d = ops.cast_rays_camera(cam, poses)                                     # whole images, no index
    assert o.shape == (K * CR.H * CR.W, 3)
    per = CR.H * CR.W
    for k in range(K):
        lo, ld = ops.cast_rays(CR.H, CR.W, CR.LEGACY_FOCAL, poses[k, :, :3].cpu(), poses[k, :, 3].cpu(), DEV)
        assert torch.equal(o[k * per:(k + 1) * per], lo) and np.array_equal(bits(d[k * per:(k + 1) * per]), bits(ld))
    # a plain (height, width, focal) tuple is that camera
    o2, d2 = ops.cast_rays_camera((CR.H, CR.W, CR.LEGACY_FOCAL), poses)
    assert torch.equal(o, o2) and torch.equal(d, d2)
    o, d = ops.cast_rays_camera(cam, poses, torch.zeros((0,), dtype=torch.int64, device=DEV))      # B == 0
    assert o.shape == (0, 3) and d.shape == (0, 3)


# ---- 2: intrinsics without distortion: the float32 restatement's bits ----------------------------------------------------
def test_undistorted_camera_matches_the_float32_restatement_bit_for_bit(scene):
    one = np.array([2 * CR.H * CR.W + 35 * CR.W + 47], dtype=np.int64)
    for idx in (None, scene["idx"], one):
        o, d = ops.cast_rays_camera(struct(CR.CAM_B), scene["poses_t"], None if idx is None else torch.from_numpy(idx).to(DEV))
        ro, rd = CR.cast_rays(CR.CAM_B, scene["poses"], idx, np.float32)
        assert rd.dtype == np.float32 and np.array_equal(bits(o), ro.view(np.uint32)) and np.array_equal(bits(d), rd.view(np.uint32))
    # not the legacy camera's rays
    la = ops.cast_rays_camera(struct(CR.CAM_A), scene["poses_t"])[1]
    assert not torch.equal(la, ops.cast_rays_camera(struct(CR.CAM_B), scene["poses_t"])[1])


# ---- 3: distortion, forward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c", "d"])
def test_distorted_forward_against_float64(scene, name):
    cam = CAMERAS[name]
    whole_o, whole_d = ops.cast_rays_camera(struct(cam), scene["poses_t"])
    o, d = ops.cast_rays_camera(struct(cam), scene["poses_t"], scene["idx_t"])
    for got_o, got_d, idx in ((whole_o, whole_d, None), (o, d, scene["idx"])):
        ref_o, ref_d = CR.cast_rays(cam, scene["poses"], idx)
        f32_d = CR.cast_rays(cam, scene["poses"], idx, np.float32)[1]
        err = float(np.abs(got_d.cpu().numpy().astype(np.float64) - ref_d).max())
        yard = float(np.abs(f32_d.astype(np.float64) - ref_d).max())
        print(f"camera ({name}) {'whole images' if idx is None else 'indexed'}: max |rays_d - float64| {err:.3e}  (float32 "
              f"restatement {yard:.3e}, bound {FWD_BOUND:.3e})")
        assert err <= FWD_BOUND and yard <= FWD_RESTATEMENT_ERR
        assert np.array_equal(got_o.cpu().numpy(), ref_o.astype(np.float32))
    # the distortion does something: far more than the bound away from the same camera without it
    plain = ops.cast_rays_camera(struct(cam._replace(dist=(0.0,) * 5)), scene["poses_t"])[1]
    assert float((plain - whole_d).abs().max()) > 1e-3
    # a ray's bits depend on that ray only: duplicates agree, and the indexed batch equals the whole images at the same pixels
    idx = scene["idx"]
    order = np.argsort(idx, kind="stable")
    same = order[1:][idx[order][1:] == idx[order][:-1]]
    prev = order[:-1][idx[order][1:] == idx[order][:-1]]
    assert len(same) >= 2 and np.array_equal(bits(d)[same], bits(d)[prev])
    assert np.array_equal(bits(d), bits(whole_d[scene["idx_t"]])) and torch.equal(o, whole_o[scene["idx_t"]])
    one = scene["idx_t"][17:18].clone()
    assert np.array_equal(bits(ops.cast_rays_camera(struct(cam), scene["poses_t"], one)[1]), bits(whole_d[one]))


# ---- 4: backward ---------------------------------------------------------------------------------------------------------
def _bwd(cam, scene, idx, g_o, g_d, **kw):
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)   # noqa: E731
    return ops.cast_rays_camera_bwd(struct(cam), scene["poses_t"], t(idx), t(g_o), t(g_d), **kw)


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("batch", ["whole", "indexed"])
def test_backward_against_float64(scene, name, batch):
    cam = CAMERAS[name]
    idx = None if batch == "whole" else scene["idx"]
    B = K * cam.H * cam.W if idx is None else len(idx)
    g_o, g_d = upstream(B)
    want = CR.cast_rays_bwd(cam, scene["poses"], idx, g_o, g_d)
    f32 = CR.cast_rays_bwd(cam, scene["poses"], idx, g_o, g_d, np.float32)
    got = [t.cpu().numpy().astype(np.float64) for t in _bwd(cam, scene, idx, g_o, g_d, want_intrinsics=True, want_distortion=True)]
    err_p = rel_l2(got[0], want[0])
    print(f"camera ({name}) {batch}: d_poses rel_l2 {err_p:.3e} (bound {POSE_GRAD_REL_L2:.0e})")
    assert err_p <= POSE_GRAD_REL_L2
    names = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
    g, w, y = np.concatenate(got[1:]), np.concatenate(want[1:]), np.concatenate(f32[1:])
    for n, gi, wi, yi in zip(names, g, w, y):
        print(f"    d_{n}: {gi:+.8e}  float64 {wi:+.8e}  |err| / |float64| {abs(gi - wi) / max(abs(wi), 1e-300):.3e}  (float32 "
              f"restatement {abs(yi - wi) / max(abs(wi), 1e-300):.3e}, bound {LENS_GRAD_BOUND:.2e})")
    for n, gi, wi, yi in zip(names, g, w, y):
        assert abs(gi - wi) <= LENS_GRAD_BOUND * abs(wi), n
        assert abs(yi - wi) <= LENS_GRAD_RESTATEMENT_ERR * abs(wi) * 1.0000001, n
    if cam.distorted:
        assert all(abs(v) > 1e-3 for v in w)                                   # no vacuous comparison
    else:
        assert all(v == 0.0 for v in g[4:])                                    # no lens: exact zeros
    if name == "a":
        # the legacy call on the same rays: d_poses, and d_focal = d_fx + d_fy
        t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)   # noqa: E731
        lp, lf = ops.cast_rays_bwd(cam.H, cam.W, CR.LEGACY_FOCAL, scene["poses_t"], t(idx), t(g_o), t(g_d), want_focal=True)
        assert rel_l2(got[0], lp.cpu().numpy()) <= POSE_GRAD_REL_L2
        assert abs((g[0] + g[1]) - float(lf)) <= POSE_GRAD_REL_L2 * abs(float(lf))


def test_backward_semantics(scene):
    cam = CR.CAM_D
    # cameras 0 and 2 only: camera 1 has no ray
    per = cam.H * cam.W
    rng = np.random.default_rng(3)
    idx = np.concatenate([rng.integers(0, per, 300), 2 * per + rng.integers(0, per, 300)]).astype(np.int64)
    rng.shuffle(idx)
    g_o, g_d = upstream(len(idx))
    want = CR.cast_rays_bwd(cam, scene["poses"], idx, g_o, g_d)
    base = _bwd(cam, scene, idx, g_o, g_d, want_intrinsics=True, want_distortion=True)
    assert int(base[0][1].count_nonzero()) == 0 and int(base[0][0].count_nonzero()) == 12          # no ray: an exact 0
    assert rel_l2(base[0].cpu().numpy(), want[0]) <= POSE_GRAD_REL_L2

    def close(a, b, bound=LENS_GRAD_BOUND):
        a, b = a.cpu().numpy().astype(np.float64), np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, np.float64)
        return bool(np.all(np.abs(a - b) <= bound * np.abs(b) + 1e-30))

    assert close(base[1], want[1]) and close(base[2], want[2])
    # garbage in the buffers does not matter without accumulate; with it the call adds
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # noqa: E731
    over = _bwd(cam, scene, idx, g_o, g_d, d_poses=nan(K, 3, 4), d_intrinsics=nan(4), d_distortion=nan(5))
    for a, b in zip(over, base):
        assert bool(torch.isfinite(a).all()) and close(a, b, 1e-6)
    ones = lambda *s: torch.ones(s, device=DEV)   # noqa: E731
    acc = _bwd(cam, scene, idx, g_o, g_d, d_poses=ones(K, 3, 4), d_intrinsics=ones(4), d_distortion=ones(5), accumulate=True)
    for a, b in zip(acc, base):
        assert float(((a - 1.0) - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1.0)
    assert bool((acc[0][1] == 1.0).all())
    # every NULL combination of the outputs: what is asked for agrees with the full call, what is not is None
    for wp, wi, wd in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        out = _bwd(cam, scene, idx, g_o, g_d, want_poses=wp, want_intrinsics=wi, want_distortion=wd)
        for got, full, wanted in zip(out, base, (wp, wi, wd)):
            assert (got is not None) == wanted
            if wanted:
                assert close(got, full, 1e-6)
    assert _bwd(cam, scene, idx, g_o, g_d, want_poses=False) == (None, None, None)                  # all NULL: nothing to do
    # either upstream gradient NULL == that gradient 0
    only_o = _bwd(cam, scene, idx, g_o, None, want_intrinsics=True, want_distortion=True)
    assert int(only_o[0][:, :, :3].count_nonzero()) == 0 and int(only_o[1].count_nonzero()) == 0 and int(only_o[2].count_nonzero()) == 0
    assert rel_l2(only_o[0][:, :, 3].cpu().numpy(), want[0][:, :, 3]) <= POSE_GRAD_REL_L2
    only_d = _bwd(cam, scene, idx, None, g_d, want_intrinsics=True, want_distortion=True)
    assert int(only_d[0][:, :, 3].count_nonzero()) == 0 and close(only_d[1], base[1], 1e-6) and close(only_d[2], base[2], 1e-6)
    zero = _bwd(cam, scene, idx, None, None, want_intrinsics=True, want_distortion=True)
    assert all(int(t.count_nonzero()) == 0 for t in zero)
    # B == 1 and B == 0
    single = _bwd(cam, scene, idx[:1], g_o[:1], g_d[:1], want_intrinsics=True, want_distortion=True)
    w1 = CR.cast_rays_bwd(cam, scene["poses"], idx[:1], g_o[:1], g_d[:1])
    assert rel_l2(single[0].cpu().numpy(), w1[0]) <= POSE_GRAD_REL_L2 and close(single[1], w1[1]) and close(single[2], w1[2])
    empty = _bwd(cam, scene, idx[:0], g_o[:0], g_d[:0], d_poses=nan(K, 3, 4), d_intrinsics=nan(4), d_distortion=nan(5))
    assert all(int(t.count_nonzero()) == 0 for t in empty)
    kept = _bwd(cam, scene, idx[:0], g_o[:0], g_d[:0], d_poses=ones(K, 3, 4), d_intrinsics=ones(4), d_distortion=ones(5), accumulate=True)
    assert all(bool((t == 1.0).all()) for t in kept)


def test_error_codes(scene):
    L = lib()
    cam, poses, idx = struct(CR.CAM_C), scene["poses_t"], scene["idx_t"]
    B = int(idx.shape[0])
    g = torch.zeros((B, 3), device=DEV)
    out, sc = torch.zeros((K, 3, 4), device=DEV), torch.zeros(4096, dtype=torch.uint8, device=DEV)
    need = L.voxe_cast_rays_camera_bwd_scratch_bytes(K)
    assert (12 * K + 9) * 8 <= need <= sc.numel()

    def bwd(c=cam, nbytes=need, scratch=sc.data_ptr()):
        return L.voxe_cast_rays_camera_bwd(ctypes.byref(c), poses.data_ptr(), K, idx.data_ptr(), B, g.data_ptr(), g.data_ptr(),
                                           out.data_ptr(), None, None, 0, scratch, nbytes, None)

    assert bwd() == abi.OK
    assert bwd(nbytes=need - 1) == abi.ERR_WORKSPACE and bwd(scratch=None) == abi.ERR_WORKSPACE
    for field, value in (("fx", 0.0), ("fy", -1.0), ("fx", float("inf")), ("fy", float("nan")), ("cx", float("nan")),
                         ("k1", float("inf")), ("k3", float("nan")), ("H", 0), ("W", -3)):
        bad = struct(CR.CAM_C)
        setattr(bad, field, value)
        assert bwd(c=bad) == abi.ERR_BAD_SHAPE, field
        assert L.voxe_cast_rays_camera(ctypes.byref(bad), poses.data_ptr(), K, idx.data_ptr(), B, g.data_ptr(), g.data_ptr(),
                                       None) == abi.ERR_BAD_SHAPE, field
        with pytest.raises(VoxeError):
            ops.cast_rays_camera(bad, poses, idx)
    torch.cuda.synchronize()


# ---- the autograd function on its own ------------------------------------------------------------------------------------
def test_cast_rays_from_camera_forward_bits_and_gradients(scene):
    """ops.cast_rays_from_camera: the forward's bits are cast_rays_camera's; poses, intrinsics [4] and distortion [5] receive the
    gradients of voxe_cast_rays_camera_bwd (bounds of test 4), each only when it asks for one"""
    cam = CR.CAM_D
    idx, g_o, g_d = scene["idx"], *upstream(len(scene["idx"]))
    want = CR.cast_rays_bwd(cam, scene["poses"], idx, g_o, g_d)
    t_o, t_d = torch.from_numpy(g_o).to(DEV), torch.from_numpy(g_d).to(DEV)
    poses = scene["poses_t"].clone().requires_grad_(True)
    intr = torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy], dtype=torch.float32, requires_grad=True)            # (host tensors: tiny)
    dist = torch.tensor(cam.dist, dtype=torch.float32, device=DEV, requires_grad=True)
    # the tensors' values replace the camera's own: start from another camera
    ro, rd = ops.cast_rays_from_camera(struct(CR.CAM_A), poses, scene["idx_t"], intrinsics=intr, distortion=dist)
    o, d = ops.cast_rays_camera(struct(cam), scene["poses_t"], scene["idx_t"])
    assert torch.equal(ro, o) and torch.equal(rd, d)
    ((ro * t_o).sum() + (rd * t_d).sum()).backward()
    assert rel_l2(poses.grad.cpu().numpy(), want[0]) <= POSE_GRAD_REL_L2
    assert intr.grad.device.type == "cpu" and dist.grad.device == dist.device
    for got, ref in ((intr.grad, want[1]), (dist.grad, want[2])):
        assert np.all(np.abs(got.cpu().numpy().astype(np.float64) - ref) <= LENS_GRAD_BOUND * np.abs(ref))
    # only the intrinsics ask: nothing else gets a gradient
    intr2 = intr.detach().clone().requires_grad_(True)
    ro, rd = ops.cast_rays_from_camera(struct(cam), scene["poses_t"], scene["idx_t"], intrinsics=intr2)
    (rd * t_d).sum().backward()
    assert np.all(np.abs(intr2.grad.numpy().astype(np.float64) - want[1]) <= LENS_GRAD_BOUND * np.abs(want[1]))
    # a PinholeCamera is a camera too
    from thre3d_atom.utils.imaging_utils import PinholeCamera

    o2, d2 = ops.cast_rays_camera(PinholeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.dist), scene["poses_t"], scene["idx_t"])
    assert torch.equal(o2, o) and torch.equal(d2, d)


def test_model_cast_rays_dispatches_on_the_camera(scene):
    """rendering/volumetric/utils/misc.cast_rays: a plain CameraIntrinsics or a legacy PinholeCamera takes voxe_cast_rays, a
    general one voxe_cast_rays_camera"""
    from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, sample_random_rays_and_pixels_from_cameras
    from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose, PinholeCamera

    p = scene["poses_t"][1]
    pose = CameraPose(p[:, :3].cpu(), p[:, 3:].cpu())
    legacy = cast_rays(CameraIntrinsics(CR.H, CR.W, CR.LEGACY_FOCAL), pose, DEV)
    same = cast_rays(PinholeCamera(CR.H, CR.W, CR.LEGACY_FOCAL), pose, DEV)
    assert torch.equal(legacy.directions, same.directions) and legacy.directions.shape == (CR.H, CR.W, 3)
    cam = CR.CAM_C
    general = cast_rays(PinholeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.dist), pose, DEV)
    want = ops.cast_rays_camera(struct(cam), scene["poses_t"][1:2])
    assert torch.equal(general.directions.reshape(-1, 3), want[1]) and torch.equal(general.origins.reshape(-1, 3), want[0])
    assert general.image_shape == (CR.H, CR.W)
    # the trainers' batch sampler
    images = torch.rand((K, 3, CR.H, CR.W), generator=torch.Generator().manual_seed(0)).to(DEV)
    torch.manual_seed(4)
    rays, pixels = sample_random_rays_and_pixels_from_cameras(PinholeCamera(cam.H, cam.W, cam.fx, cam.fy, cam.cx, cam.cy, cam.dist),
                                                              scene["poses_t"], images, 500)
    torch.manual_seed(4)
    subset = torch.randperm(K * CR.H * CR.W, dtype=torch.long, device=DEV)[:500]
    want = ops.cast_rays_camera(struct(cam), scene["poses_t"], subset)
    assert torch.equal(rays.directions, want[1]) and pixels.shape == (500, 3)


# ---- 7: dataset routing --------------------------------------------------------------------------------------------------
def test_trainer_routes_general_cameras_to_the_composed_iteration(tmp_path, monkeypatch):
    """a dataset with a general camera trains on the composed path (cast_rays_camera, render, step) and never calls the one-call
    iteration (ops.recon_step_), which casts (height, width, focal) cameras only; the legacy dataset still calls it"""
    import logging

    from thre3d_atom.data.datasets import InMemoryPosedImages
    from thre3d_atom.modules import optim
    from thre3d_atom.modules.trainers import train_sh_vox_grid_vol_mod_with_posed_images
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraIntrinsics, PinholeCamera, pose_spherical
    from thre3d_atom.utils.logging import log

    calls = {"recon": 0, "camera": 0}
    real_recon, real_cast = optim._ops.recon_step_, ops.cast_rays_camera

    def counted_recon(*a, **kw):
        calls["recon"] += 1
        return real_recon(*a, **kw)

    def counted_cast(*a, **kw):
        calls["camera"] += 1
        return real_cast(*a, **kw)

    monkeypatch.setattr(optim._ops, "recon_step_", counted_recon)
    monkeypatch.setattr(ops, "cast_rays_camera", counted_cast)
    h, w = 24, 32
    g = torch.Generator().manual_seed(2)
    images = torch.rand((4, 3, h, w), generator=g)
    poses = torch.stack([torch.cat(pose_spherical(90.0 * i, 40.0, 4.0311), dim=1) for i in range(4)])

    class Capture(logging.Handler):
        lines = []

        def emit(self, record):
            self.lines.append(record.getMessage())

    def run(camera, out):
        vg = VoxelGrid(torch.empty(24, 24, 24, 1).uniform_(-1, 1, generator=g), torch.empty(24, 24, 24, 3).uniform_(-1, 1, generator=g),
                       VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                       density_postactivation=torch.nn.Softplus(), expected_density_scale=100.0 / 3.0, tunable=True)
        vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(64, CameraBounds(1.8, 6.6), white_bkgd=True), device=DEV)
        calls["recon"] = calls["camera"] = 0
        cap = Capture()
        cap.lines = []
        log.addHandler(cap)
        try:
            train_sh_vox_grid_vol_mod_with_posed_images(vm, InMemoryPosedImages(images, poses, camera, CameraBounds(1.8, 6.6)), out,
                                                        random_initializer=lambda t: t, ray_batch_size=1024, num_stages=1,
                                                        num_iterations_per_stage=2, summary_freq=1, fast_debug_mode=True)
        finally:
            log.removeHandler(cap)
        before = vg.densities.detach().clone()
        assert bool(torch.isfinite(vm.thre3d_repr.densities).all())
        return dict(calls), cap.lines, vm, before

    general = PinholeCamera(h, w, 40.0, 37.0, 15.2, 12.6, (-0.12, 0.03, 0.002, -0.001, 0.0))
    n, lines, vm, _ = run(general, tmp_path / "general")
    assert n["recon"] == 0 and n["camera"] == 2
    assert sum("no one-call iteration" in line and "general camera" in line for line in lines) == 1             # said once
    saved = torch.load(tmp_path / "general" / "saved_models" / "model_final.pth", map_location="cpu", weights_only=False)
    assert general in [v for v in saved.values() if isinstance(v, PinholeCamera)] or general in [
        v for d in saved.values() if isinstance(d, dict) for v in d.values() if isinstance(v, PinholeCamera)]
    n, lines, _, _ = run(CameraIntrinsics(h, w, 40.0), tmp_path / "legacy")
    assert n["recon"] == 2 and n["camera"] == 0 and not any("general camera" in line for line in lines)
    n, _, _, _ = run(PinholeCamera(h, w, 40.0), tmp_path / "legacy_pinhole")                                # a legacy PinholeCamera too
    assert n["recon"] == 2 and n["camera"] == 0


# ---- 5: autograd wiring through a render ---------------------------------------------------------------------------------
def _recovery_scene():
    import synth

    dens, feat = CR.recovery_grid()
    spec = ops.GridSpec(aabb=((-1.5, 1.5),) * 3, density_scale=CR.RECOVERY_DENSITY_SCALE, density_pre_act=abi.ACT_IDENTITY,
                        density_post_act=abi.ACT_SOFTPLUS)
    params = ops.RenderParams(num_samples=CR.RECOVERY_SAMPLES, near=synth.NEAR, far=synth.FAR, white_bkgd=True,
                              image_width=CR.SMALL_W, image_height=CR.SMALL_H)
    return spec, params, dens.to(DEV), feat.to(DEV), CR.recovery_poses().to(DEV)


def test_intrinsics_gradient_through_a_render_against_central_differences():
    """d sum(colour . fixed weights) / d (fx, fy, cx, cy) through cast_rays_from_camera -> ops.render (voxe_render_bwd_rays ->
    voxe_cast_rays_camera_bwd) against central differences of the same GPU forward; camera (c) at 32 x 24, 4 poses, the 24^3 SH-0
    sphere of tests/synth.py.
    Bound per component: 0.05 max|gradient| + noise.  The forward is float32: each colour carries about 1e-6 of rounding (the
    suite holds colours to 1e-5 of the oracle, smoke() measures 2.4e-7), so the difference of two sums of N = 9216 weighted
    colours (weights U(0,1), mean square 1/3) is uncertain by sqrt(2 N / 3) 1e-6 = 7.8e-5, divided by 2 h.  The render is
    piecewise trilinear in the ray: a central difference over +-h smooths the kinks that the analytic gradient samples at a
    point, an error proportional to h times the density of kinks; h is 2e-3 of the focal lengths and 0.05 px for the centre
    (0.07 / 0.06 / 0.05 / 0.05), about 1.5e-3 in normalised coordinates, 1/80 of a voxel at the object.  5 % of the largest
    component is the allowance for that; a wrong sign, a swapped component or a factor fx in the chain is off by 100 %.
    Measured (autograd / central differences): fx -18.03 / -18.95, fy -21.44 / -22.09, cx -2.34 / -3.42, cy -13.2834 / -13.2835;
    bound 1.11 per component."""
    spec, params, dens, feat, poses = _recovery_scene()
    cam = CR.CAM_C_SMALL
    weights = torch.rand((4 * cam.H * cam.W, 3), generator=torch.Generator().manual_seed(12)).to(DEV)
    truth = CR.recovery_truth()

    def forward(values, grad=False):
        intr = torch.tensor(values, dtype=torch.float32, requires_grad=grad)
        ro, rd = ops.cast_rays_from_camera(struct(cam), poses, None, intrinsics=intr)
        colour = ops.render(spec, params, dens, feat, ro, rd)[0]
        return intr, colour

    intr, colour = forward(truth, grad=True)
    (colour * weights).sum().backward()
    got = intr.grad.double().numpy()
    steps = np.array([2e-3 * truth[0], 2e-3 * truth[1], 0.05, 0.05])
    noise = np.sqrt(2 * weights.numel() / 3.0) * 1e-6
    fd = np.zeros(4)
    with torch.no_grad():
        for j in range(4):
            vals = []
            for sign in (+1.0, -1.0):
                v = truth.copy()
                v[j] += sign * steps[j]
                vals.append(float((forward(v)[1].double() * weights.double()).sum()))
            fd[j] = (vals[0] - vals[1]) / (2 * steps[j])
    bound = 0.05 * np.abs(fd).max() + noise / (2 * steps)
    for n, g, f, b in zip(("fx", "fy", "cx", "cy"), got, fd, bound):
        print(f"d_{n}: autograd {g:+.5e}  central differences {f:+.5e}  |diff| {abs(g - f):.2e}  bound {b:.2e}")
    assert np.abs(fd).max() > 20 * (noise / (2 * steps)).max()                    # the comparison is above the noise
    assert np.all(np.abs(got - fd) <= bound)


# ---- 6: intrinsics refinement end to end ---------------------------------------------------------------------------------
def test_intrinsics_refinement_recovers_the_camera(tmp_path):
    """refine_camera_poses(..., intrinsics_learning_rate) on targets rendered with camera (c) at 32 x 24 from 4 exact poses, grid
    frozen, start fx, fy + 3 % and cx, cy + 1.5 px, 100 Adam steps at 0.05.  The float64 restatement of the same problem
    (camera_ref.recovery_float64, same camera draws) ends at 0.01416 of its initial intrinsic error (loss 1.894e-2 -> 1.643e-6);
    the GPU run must end within 1.5 x that ratio with its loss below its starting loss.  Measured: 0.01416, 1.894e-2 -> 1.643e-6."""
    import json

    from thre3d_atom.data.datasets import InMemoryPosedImages, camera_from_params
    from thre3d_atom.modules.pose_refiner import refine_camera_poses
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds, CameraPose, PinholeCamera

    import synth

    dens, feat = CR.recovery_grid()
    vg = VoxelGrid(dens, feat, VoxelSize(0.125, 0.125, 0.125), density_preactivation=torch.nn.Identity(),
                   density_postactivation=torch.nn.Softplus(), expected_density_scale=CR.RECOVERY_DENSITY_SCALE, tunable=True)
    bounds = CameraBounds(synth.NEAR, synth.FAR)
    vm = VolumetricModel(vg, render_sh_voxel_grid, SHVoxGridRenderConfig(CR.RECOVERY_SAMPLES, bounds, white_bkgd=True,
                                                                         render_num_samples_per_ray=CR.RECOVERY_SAMPLES), device=DEV)
    c = CR.CAM_C_SMALL
    true_cam = PinholeCamera(c.H, c.W, c.fx, c.fy, c.cx, c.cy, c.dist)
    poses = CR.recovery_poses()
    images = torch.stack([vm.render(CameraPose(p[:, :3], p[:, 3:]), true_cam, gpu_render=True, verbose=False,
                                    perturb_sampled_points=False).colour.permute(2, 0, 1).cpu() for p in poses])
    start = true_cam.with_intrinsics(*CR.recovery_start())
    data = InMemoryPosedImages(images, poses, start, bounds)
    learned = {}
    torch.manual_seed(CR.RECOVERY_SEED)
    refined, losses = refine_camera_poses(vm, data, tmp_path, num_iterations=CR.RECOVERY_STEPS, ray_batch_size=4 * c.H * c.W,
                                          image_batch_cache_size=4, summary_freq=1, intrinsics_learning_rate=CR.RECOVERY_LR,
                                          pose_learning=False, learned=learned)
    cam = learned["camera"]
    end = np.array([cam.fx, cam.fy, cam.cx, cam.cy]) - CR.recovery_truth()
    ratio = float(np.linalg.norm(end) / np.linalg.norm(CR.recovery_start() - CR.recovery_truth()))
    print(f"intrinsics recovery: |error| ratio {ratio:.5f} (float64 run {CR.RECOVERY_RATIO_FLOAT64}, bound "
          f"{1.5 * CR.RECOVERY_RATIO_FLOAT64:.5f}); loss {losses[0]:.3e} -> {losses[-1]:.3e}; camera {cam}")
    assert len(losses) == CR.RECOVERY_STEPS and losses[-1] < losses[0]
    assert ratio <= 1.5 * CR.RECOVERY_RATIO_FLOAT64
    assert torch.equal(refined.cpu(), poses) and cam.distortion == true_cam.distortion     # poses exact, coefficients fixed
    written = json.loads((tmp_path / "refined_train_camera_params.json").read_text())      # the written file carries the camera
    assert camera_from_params(written, sorted(written)[0]) == cam
