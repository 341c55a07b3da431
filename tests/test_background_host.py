"""CPU checks of the environment-map background: self-checks of the float64 restatement tests/background_ref.py (its analytic
gradients against autograd, its direction constructor, that the case tables of the GPU tests are not vacuous), the C ABI's
declarations and argument validation (no device work), the command-line options, the trainer's arguments and the checkpoint
round trip."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest
import torch

import background_ref as BR
from conftest import GOLDEN, ROOT
from voxe_hip import abi

CPU = torch.device("cpu")


# ---- the restatement checks itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("He,We", BR.MAPS)
def test_analytic_gradients_agree_with_autograd(He, We):
    texels, d, colour, acc, g, _, _ = BR.agreement_case(He, We, 4096)
    # (+ the conventions: the two poles, a zero-length and a non-finite direction)
    d = torch.cat([d, torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, -0.5], [0.0, 0.0, 0.0], [float("nan"), 1.0, 0.0]])])
    pad = lambda t: torch.cat([t, t[:4]])
    colour, acc, g = pad(colour), pad(acc), pad(g)
    out, a_acc, a_tex, a_d = BR.autograd_gradients(colour, acc, d, texels, g)
    d_acc, d_tex, d_d, s = BR.analytic_gradients(acc, d, texels, g)
    for name, got, want in (("d_acc", d_acc, a_acc), ("d_texels", d_tex, a_tex), ("d_rays_d", d_d, a_d)):
        err = BR.rel_l2(got, want)
        print(f"{He}x{We} {name}: rel_l2 {err:.3e}")
        assert err < 1e-12, (name, err)
    assert torch.equal(d_d[-4:], torch.zeros(4, 3, dtype=torch.float64))        # poles and unusable directions: exactly 0
    assert torch.equal(out[-2:], colour[-2:].double()) and float(s[-2:].abs().max()) == 0.0      # unusable: b = 0
    assert bool((out[-4:-2] != colour[-4:-2].double()).any())                   # the poles still have a value
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("He,We", BR.MAPS)
def test_constructed_directions_map_back(He, We):
    _, _, _, _, _, u, v = BR.agreement_case(He, We, 4096)
    length = torch.linspace(0.25, 4.0, 4096, dtype=torch.float64)
    d = BR.directions_from_uv(u, v, He, We, length)
    u2, v2, usable = BR.map_coords(d, He, We)
    assert bool(usable.all())
    assert float((u2 - u).abs().max()) < 1e-9 and float((v2 - v).abs().max()) < 1e-9
    assert float((d.norm(dim=1) - length).abs().max()) < 1e-12


@pytest.mark.parametrize("He,We", BR.MAPS)
@pytest.mark.parametrize("R", BR.RAY_COUNTS)
def test_agreement_cases_are_not_vacuous(He, We, R):
    texels, d, colour, acc, g, u, v = BR.agreement_case(He, We, R)
    u32, v32, usable = BR.map_coords(d.double(), He, We)                        # what the float32 directions map to
    assert bool(usable.all())
    for f in (u32 - torch.floor(u32), v32 - torch.floor(v32)):
        assert float(f.min()) >= 0.05 - 1e-5 and float(f.max()) <= 0.95 + 1e-5   # no ray on a cell boundary
    assert torch.equal(torch.floor(u32), torch.floor(u)) and torch.equal(torch.floor(v32), torch.floor(v))
    norm = d.double().norm(dim=1)
    assert float(norm.min()) >= 0.24 and float(norm.max()) <= 4.1
    if R < 4096:
        return
    _, _, _, _, x0, y0 = BR.taps(u32, v32, He, We)
    ck, rk = BR.tap_kinds(x0, y0, He, We)
    kinds = set(zip(ck.tolist(), rk.tolist()))
    want = {(c, r) for c in (0, 1, 2) for r in (0, 1, 2)}    # (2 texels: x0 = 0 is the interior cell, its second tap the last column)
    assert kinds == want, sorted(want - kinds)
    assert int((acc == 0).sum()) > 10 and int((acc == 1).sum()) > 10 and int((g == 0).all(dim=1).sum()) > 10
    _, d_tex, d_d, s = BR.analytic_gradients(acc, d, texels, g)
    assert int((s == 0).all(dim=1).sum()) > 20 and int((d_tex != 0).sum()) == d_tex.numel()
    assert float(d_d.norm()) > 0 and float(norm.std()) > 0.5


def test_contention_cases_are_what_they_claim():
    for case, lo, hi in ((BR.one_cell_case(), 4096, 4096), (BR.two_cell_case(), 1, 1), (BR.camera_case(), 1, 2304)):
        texels, d = case[0], case[1]
        runs = BR.run_lengths(d, *texels.shape[:2])
        assert int(runs.min()) >= lo and int(runs.max()) <= hi
    runs = BR.run_lengths(BR.camera_case()[1], 4, 8)
    assert float(runs.float().mean()) > 8 and len(runs) > 48          # long runs, and more than one cell per image row


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
NAMES = ("voxe_background_fwd", "voxe_background_bwd", "voxe_background_debug_merge")


def _lib():
    from voxe_hip import build

    return abi.declare(ctypes.CDLL(build.build()), "voxe_")


def test_background_symbols_are_declared_with_no_cpu_twin_and_abi_13():
    text = open(os.path.join(ROOT, "include", "voxe.h")).read()
    L = _lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text) and name in abi.hip_symbols() and hasattr(L, name)
    assert not re.search(r"\bvoxe_cpu_\w*background", text)
    assert not any("background" in s for s in abi.cpu_symbols())
    assert abi.ABI_VERSION == 13 and "#define VOXE_ABI_VERSION 13" in text and L.voxe_abi_version() == 13
    assert "voxe_background.hip" in __import__("voxe_hip.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(ROOT, "vox-e_amd", "csrc", "voxe_background.hip")).read()
    assert "getenv" not in src and "ds_add_f32" not in src
    for name, want in (("voxe_background_fwd", ["env", "rays_d", "R", "colour_in", "acc", "colour_out", "stream"]),
                       ("voxe_background_bwd", ["env", "rays_d", "R", "acc", "d_colour_out", "d_acc", "d_texels", "d_rays_d",
                                                "accumulate", "stream"])):
        proto = re.search(rf"int {name}\((.*?)\);", text, re.S).group(1)
        proto = re.sub(r"/\*.*?\*/", "", proto, flags=re.S)
        assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == want
        assert len(getattr(L, name).argtypes) == len(want)


def test_env_map_layout_matches_header(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxe.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   "sizeof(VoxeEnvMap), offsetof(VoxeEnvMap, texels), offsetof(VoxeEnvMap, height), offsetof(VoxeEnvMap, width)); "
                   "return 0; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E = abi.VoxeEnvMap
    assert vals == [ctypes.sizeof(E), E.texels.offset, E.height.offset, E.width.offset]


def test_validation_without_a_device():
    L = _lib()
    P = ctypes.c_void_p(16)

    def env(h=4, w=8, texels=16):
        e = abi.VoxeEnvMap()
        e.texels, e.height, e.width = texels, h, w
        return e

    def fwd(e=env(), rd=P, R=4, ci=P, acc=P, co=P):
        return L.voxe_background_fwd(ctypes.byref(e) if e is not None else None, rd, R, ci, acc, co, None)

    def bwd(e=env(), rd=P, R=4, acc=P, g=P, d_acc=None, d_tex=None, d_rd=None, accumulate=0):
        return L.voxe_background_bwd(ctypes.byref(e) if e is not None else None, rd, R, acc, g, d_acc, d_tex, d_rd, accumulate, None)

    for call in (fwd, bwd):
        # NULL required pointers
        assert call(e=None) == abi.ERR_NULL_POINTER and call(e=env(texels=None)) == abi.ERR_NULL_POINTER
        assert call(rd=None) == abi.ERR_NULL_POINTER and call(acc=None) == abi.ERR_NULL_POINTER
        # shapes
        assert call(e=env(h=1)) == abi.ERR_BAD_SHAPE and call(e=env(w=1)) == abi.ERR_BAD_SHAPE
        assert call(e=env(h=0, w=-3)) == abi.ERR_BAD_SHAPE
        assert call(R=-1) == abi.ERR_BAD_SHAPE and call(R=1 << 31) == abi.ERR_BAD_SHAPE
        # R == 0: nothing is launched (NULL rays allowed)
        assert call(R=0) == abi.OK and call(R=0, rd=None, acc=None) == abi.OK
    assert fwd(ci=None) == abi.ERR_NULL_POINTER and fwd(co=None) == abi.ERR_NULL_POINTER
    assert bwd(g=None) == abi.ERR_NULL_POINTER
    assert bwd(R=0, d_acc=P, d_tex=P, d_rd=P) == abi.OK and bwd(R=0, d_tex=P, accumulate=1) == abi.OK
    assert bwd() == abi.OK                                                      # all three outputs NULL: no launch
    assert fwd(e=env(h=2, w=2), R=0) == abi.OK
    for mode in (1, 2, 0):
        assert L.voxe_background_debug_merge(mode) == abi.OK
    assert L.voxe_background_debug_merge(3) == abi.ERR_BAD_SHAPE and L.voxe_background_debug_merge(-1) == abi.ERR_BAD_SHAPE


def test_operator_refuses_host_tensors():
    from voxe_hip import ops
    from voxe_hip.runtime import VoxeError

    with pytest.raises(VoxeError):
        ops.background_composite(torch.zeros(2, 3), torch.zeros(2), torch.ones(2, 3), torch.zeros(4, 8, 3))
    with pytest.raises(VoxeError):
        ops.background_composite(torch.zeros(2, 3), torch.zeros(3), torch.ones(2, 3), torch.zeros(4, 8, 3))
    assert callable(ops.background_fwd_into) and callable(ops.background_bwd)


# ---- command line, trainer, checkpoint ----------------------------------------------------------------------------------------
def _entry(script):
    spec = importlib.util.spec_from_file_location("bg_cli_" + script[:-3], os.path.join(ROOT, script))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {p.name: p for p in mod.main.params}


def test_cli_options_and_trainer_arguments():
    train = _entry("train_sh_based_voxel_grid_with_posed_images.py")
    assert train["background_resolution"].default == 0 and "--background_resolution" in train["background_resolution"].opts
    assert train["background_learning_rate"].default is None and "--background_learning_rate" in train["background_learning_rate"].opts
    render = _entry("render_sh_based_voxel_grid.py")
    assert render["ignore_background"].default is False and render["ignore_background"].is_flag
    from thre3d_atom.modules import trainers
    from thre3d_atom.modules.volumetric_model import VolumetricModel

    sig = inspect.signature(trainers.train_sh_vox_grid_vol_mod_with_posed_images)
    assert sig.parameters["background_resolution"].default == 0
    assert sig.parameters["background_learning_rate"].default is None
    init = inspect.signature(VolumetricModel.__init__)
    assert list(init.parameters)[-1] == "background" and init.parameters["background"].default is None
    for fn in (VolumetricModel.render_rays, VolumetricModel.render):
        assert inspect.signature(fn).parameters["with_background"].default is True
    assert "with_background" not in inspect.signature(VolumetricModel.render_rays_attn).parameters
    for doc in ("README.md", "INTEGRATION.md"):
        assert "--background_resolution" in open(os.path.join(ROOT, doc)).read(), doc
    assert "4.15" in open(os.path.join(ROOT, "DESIGN.md")).read()


def _model(background=None, white=False):
    from thre3d_atom.modules.volumetric_model import VolumetricModel
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig, render_sh_voxel_grid
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize
    from thre3d_atom.utils.imaging_utils import CameraBounds

    vg = VoxelGrid(torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3), VoxelSize(0.1, 0.1, 0.1), tunable=True)
    cfg = SHVoxGridRenderConfig(8, CameraBounds(1.0, 4.0), white_bkgd=white)
    return VolumetricModel(vg, render_sh_voxel_grid, cfg, device=CPU, background=background)


def test_checkpoint_round_trip_and_reference_checkpoint(tmp_path):
    import dataclasses

    from thre3d_atom._keys import CHECKPOINT_KEYS
    from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model
    from thre3d_atom.thre3d_reprs.background import EnvMapBackground
    from thre3d_atom.thre3d_reprs.renderers import SHVoxGridRenderConfig
    from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict

    assert CHECKPOINT_KEYS["BACKGROUND"] == "background"
    assert "background" not in {f.name for f in dataclasses.fields(SHVoxGridRenderConfig)}
    bg = EnvMapBackground(4, 8)
    assert int(bg.texels.count_nonzero()) == 0 and bg.texels.requires_grad and bg.get_save_config_dict() == {"height": 4, "width": 8}
    with torch.no_grad():
        bg.texels.copy_(torch.randn(4, 8, 3))
    with_bg, without = _model(bg), _model()
    assert with_bg.background is bg and without.background is None
    info = with_bg.get_save_info()
    assert set(info["background"]) == {"state_dict", "config_dict"} and "background" not in without.get_save_info()
    torch.save(info, tmp_path / "with.pth")
    torch.save(without.get_save_info(), tmp_path / "without.pth")
    loaded, _ = create_volumetric_model_from_saved_model(tmp_path / "with.pth", create_voxel_grid_from_saved_info_dict, device=CPU)
    assert torch.equal(loaded.background.texels, bg.texels) and not loaded.background.texels.requires_grad
    plain, _ = create_volumetric_model_from_saved_model(tmp_path / "without.pth", create_voxel_grid_from_saved_info_dict, device=CPU)
    assert plain.background is None
    ref, _ = create_volumetric_model_from_saved_model(os.path.join(GOLDEN, "ref_checkpoint.pth"), create_voxel_grid_from_saved_info_dict,
                                                      device=CPU)
    assert ref.background is None


def test_white_background_and_a_background_model_exclude_each_other(tmp_path):
    from thre3d_atom.modules import trainers
    from thre3d_atom.thre3d_reprs.background import EnvMapBackground

    with pytest.raises(ValueError):
        _model(EnvMapBackground(4, 8), white=True)
    with pytest.raises(ValueError):
        _model(white=True).background = EnvMapBackground(4, 8)
    with pytest.raises(ValueError):
        EnvMapBackground(1, 8)
    with pytest.raises(ValueError):       # (raised before the dataset is touched)
        trainers.train_sh_vox_grid_vol_mod_with_posed_images(_model(white=True), None, tmp_path, background_resolution=8)
