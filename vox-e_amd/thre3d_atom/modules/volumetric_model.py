"""VolumetricModel: a 3-D representation + its render procedure + render config.

API of the reference's thre3d_atom/modules/volumetric_model.py (`VolumetricModel` :30-253, loaders
:256-301): `render_rays(_attn)` is differentiable, `render(_attn)` renders a whole camera without grad,
`get_save_info` produces the checkpoint dictionary.
"""
import copy
import dataclasses
from pathlib import Path
from typing import Any, Callable, Dict, Optional, Tuple

import torch
from torch.nn import Module

from thre3d_atom.rendering.volumetric.render_interface import Rays, RenderOut, RenderOutAttn
from thre3d_atom.rendering.volumetric.utils.misc import (
    cast_rays,
    collate_rendered_output,
    collate_rendered_output_attn,
    flatten_rays,
    reshape_rendered_output,
    reshape_rendered_output_attn,
)
from thre3d_atom.thre3d_reprs.constants import (
    BACKGROUND,
    CONFIG_DICT,
    EXPOSURE,
    RENDER_CONFIG,
    RENDER_CONFIG_TYPE,
    RENDER_PROCEDURE,
    STATE_DICT,
    THRE3D_REPR,
)
from thre3d_atom.thre3d_reprs.compression import COMPRESSED, expand_checkpoint_
from thre3d_atom.thre3d_reprs.renderers import RenderConfig, RenderProcedure, render_sh_voxel_grid_attn
from thre3d_atom.utils.constants import EXTRA_ACCUMULATED_WEIGHTS, EXTRA_INFO
from thre3d_atom.utils.imaging_utils import CameraIntrinsics, CameraPose


class VolumetricModel:
    def __init__(
        self,
        thre3d_repr: Module,
        render_procedure: RenderProcedure,
        render_config: RenderConfig,
        render_procedure_attn=None,
        device: torch.device = torch.device("cuda" if torch.cuda.is_available() else "cpu"),
        background: Optional[Module] = None,   # addition of this build: thre3d_reprs.background.EnvMapBackground behind the grid
    ) -> None:
        self._thre3d_repr = thre3d_repr.to(device)
        self._render_procedure = render_procedure
        self._render_procedure_attn = render_procedure_attn
        self._render_config = render_config
        self._device = device
        self._background = None
        self.background = background
        self._exposure = None   # (set through the property: the trainer and the checkpoint loader do)

    @property
    def exposure(self) -> Optional[Module]:
        """the per-image affine colour transforms of the training images (thre3d_reprs.exposure.PerImageExposure; None: the
        model has none).  It belongs to the photometric loss of the training images, not to the scene: renders are never altered
        by it"""
        return self._exposure

    @exposure.setter
    def exposure(self, exposure: Optional[Module]) -> None:
        self._exposure = None if exposure is None else exposure.to(self._device)

    @property
    def background(self) -> Optional[Module]:
        """the learned background composited behind every `render_rays` / `render` (None: black, or white_bkgd)"""
        return self._background

    @background.setter
    def background(self, background: Optional[Module]) -> None:
        if background is not None and getattr(self._render_config, "white_bkgd", False):
            raise ValueError("a background model and white_bkgd=True exclude each other: the white background is already "
                             "composited by the renderer")
        self._background = None if background is None else background.to(self._device)

    @property
    def thre3d_repr(self) -> Module:
        return self._thre3d_repr

    @thre3d_repr.setter
    def thre3d_repr(self, thre3d_repr: Module) -> None:
        self._thre3d_repr = thre3d_repr

    @property
    def render_procedure(self) -> RenderProcedure:
        return self._render_procedure

    @property
    def render_config(self) -> RenderConfig:
        return self._render_config

    @property
    def device(self) -> torch.device:
        return self._device

    @staticmethod
    def _update_render_config(render_config: RenderConfig, update_dict: Dict[str, Any]) -> RenderConfig:
        """copy of the config with `update_dict` applied; unknown fields are an error"""
        updated = copy.deepcopy(render_config)
        for name, value in update_dict.items():
            if not hasattr(updated, name):
                raise ValueError(f"Unknown render configuration field {name} requested for overriding :(")
            setattr(updated, name, value)
        return updated

    def get_save_info(self, extra_info: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        save_info = {
            THRE3D_REPR: {
                STATE_DICT: self._thre3d_repr.state_dict(),
                CONFIG_DICT: self._thre3d_repr.get_save_config_dict(),
            },
            RENDER_PROCEDURE: self._render_procedure,
            RENDER_CONFIG_TYPE: type(self._render_config),
            RENDER_CONFIG: dataclasses.asdict(self._render_config),
        }
        if self._background is not None:
            save_info[BACKGROUND] = {
                STATE_DICT: self._background.state_dict(),
                CONFIG_DICT: self._background.get_save_config_dict(),
            }
        if self._exposure is not None:
            save_info[EXPOSURE] = {
                STATE_DICT: self._exposure.state_dict(),
                CONFIG_DICT: self._exposure.get_save_config_dict(),
            }
        if extra_info is not None:
            save_info[EXTRA_INFO] = extra_info
        return save_info

    # -- differentiable ---------------------------------------------------------------------------
    def render_rays(self, rays: Rays, parallel_points_chunk_size: Optional[int] = None, with_background: bool = True,
                    **kwargs) -> RenderOut:
        config = self._update_render_config(self._render_config, kwargs)
        out = self._render_procedure(self._thre3d_repr, rays, config, parallel_points_chunk_size)
        if self._background is None or not with_background:
            return out
        if getattr(config, "white_bkgd", False):
            raise ValueError("a background model and white_bkgd=True exclude each other: the white background is already "
                             "composited by the renderer")
        # the background sees what the grid left of each ray: colour + (1 - acc) * b(direction); depth and extra stay the grid's
        colour = self._background(out.colour, out.extra[EXTRA_ACCUMULATED_WEIGHTS], rays.directions)
        return RenderOut(colour=colour, depth=out.depth, extra=out.extra)

    def render_rays_attn(
        self, rays: Rays, parallel_points_chunk_size: Optional[int] = None, orig_densities=False, **kwargs
    ) -> RenderOutAttn:
        config = self._update_render_config(self._render_config, kwargs)
        return self._render_procedure_attn(self._thre3d_repr, rays, config, parallel_points_chunk_size, orig_densities)

    def distortion_loss(self, rays: Rays, **kwargs) -> torch.Tensor:
        """mean distortion loss of flat `rays` (thre3d_reprs.distortion.distortion_loss_on_rays) under the model's render
        config with `kwargs` applied; differentiable w.r.t. the grid's densities"""
        from thre3d_atom.thre3d_reprs.distortion import distortion_loss_on_rays

        return distortion_loss_on_rays(self._thre3d_repr, rays, self._update_render_config(self._render_config, kwargs))

    def depth_loss(self, rays: Rays, target_depth: torch.Tensor, target_sigma: torch.Tensor,
                   ray_weight: Optional[torch.Tensor] = None, eps: float = 1e-5, **kwargs) -> torch.Tensor:
        """mean ray-termination loss of flat `rays` towards per-ray depth targets (thre3d_reprs.depth.depth_loss_on_rays)
        under the model's render config with `kwargs` applied; differentiable w.r.t. the grid's densities"""
        from thre3d_atom.thre3d_reprs.depth import depth_loss_on_rays

        return depth_loss_on_rays(self._thre3d_repr, rays, target_depth, target_sigma,
                                  self._update_render_config(self._render_config, kwargs), ray_weight=ray_weight, eps=eps)

    def orientation_loss(self, rays: Rays, ray_weight: Optional[torch.Tensor] = None, normal_eps: float = 1e-2,
                         **kwargs) -> torch.Tensor:
        """mean orientation loss of flat `rays` (thre3d_reprs.orientation.orientation_loss_on_rays) under the model's render
        config with `kwargs` applied; differentiable w.r.t. the grid's densities"""
        from thre3d_atom.thre3d_reprs.orientation import orientation_loss_on_rays

        return orientation_loss_on_rays(self._thre3d_repr, rays, self._update_render_config(self._render_config, kwargs),
                                        ray_weight=ray_weight, normal_eps=normal_eps)

    # -- whole-camera, no grad --------------------------------------------------------------------
    def _render_camera(self, render_chunk, collate, reshape, camera_pose, camera_intrinsics,
                       parallel_rays_chunk_size, gpu_render, verbose):
        flat_rays = flatten_rays(cast_rays(camera_intrinsics, camera_pose, device=self._device))
        # The reference loops over chunks of `parallel_rays_chunk_size` rays (default 32768) only to
        # bound its [rays x samples] temporaries (volumetric_model.py:170-186).  The fused kernel has no
        # such temporaries, so the whole image is ONE launch (2-D pixel tiles, XCD-banded); the chunk
        # size is a memory knob without numerical meaning and is accepted but not used.
        del parallel_rays_chunk_size, verbose
        with torch.no_grad():
            chunks = [render_chunk(flat_rays)]
            if not gpu_render:
                chunks = [c.to(torch.device("cpu")) for c in chunks]
        return reshape(collate(chunks), camera_intrinsics=camera_intrinsics)

    def render(
        self,
        camera_pose: CameraPose,
        camera_intrinsics: CameraIntrinsics,
        parallel_rays_chunk_size: Optional[int] = 32768,
        parallel_points_chunk_size: Optional[int] = None,
        gpu_render: bool = True,
        verbose: bool = False,
        with_background: bool = True,
        **kwargs,
    ) -> RenderOut:
        return self._render_camera(
            lambda r: self.render_rays(r, parallel_points_chunk_size, with_background=with_background, **kwargs),
            collate_rendered_output, reshape_rendered_output,
            camera_pose, camera_intrinsics, parallel_rays_chunk_size, gpu_render, verbose,
        )

    def render_attn(
        self,
        camera_pose: CameraPose,
        camera_intrinsics: CameraIntrinsics,
        parallel_rays_chunk_size: Optional[int] = 32768,
        parallel_points_chunk_size: Optional[int] = None,
        gpu_render: bool = True,
        verbose: bool = False,
        orig_densities=False,
        **kwargs,
    ) -> RenderOutAttn:
        return self._render_camera(
            lambda r: self.render_rays_attn(r, parallel_points_chunk_size, orig_densities, **kwargs),
            collate_rendered_output_attn, reshape_rendered_output_attn,
            camera_pose, camera_intrinsics, parallel_rays_chunk_size, gpu_render, verbose,
        )


def _load_model(model_path: Path, make_repr, device) -> Tuple[VolumetricModel, Dict[str, Any]]:
    # checkpoints hold pickled callables/classes (render procedure, activations), which torch >= 2.6
    # refuses under its default weights_only=True
    model_data = torch.load(model_path, map_location="cpu", weights_only=False)
    if COMPRESSED in model_data[THRE3D_REPR]:
        # a compressed checkpoint: back to an ordinary state dict before the representation is made
        expand_checkpoint_(model_data)
    render_config =model_data[RENDER_CONFIG_TYPE](**model_data[RENDER_CONFIG])
    model = VolumetricModel(
        thre3d_repr=make_repr(model_data),
        render_procedure=model_data[RENDER_PROCEDURE],
        render_procedure_attn=render_sh_voxel_grid_attn,
        render_config=render_config,
        device=device,
        background=_load_background(model_data),
    )
    model.exposure = _load_exposure(model_data)
    return model, model_data.get(EXTRA_INFO)


def _load_background(model_data: Dict[str, Any]) -> Optional[Module]:
    """the checkpoint's environment-map background, frozen (None: the checkpoint has none -- every reference checkpoint)"""
    if BACKGROUND not in model_data:
        return None
    from thre3d_atom.thre3d_reprs.background import EnvMapBackground

    background = EnvMapBackground(**model_data[BACKGROUND][CONFIG_DICT])
    background.load_state_dict(model_data[BACKGROUND][STATE_DICT])
    return background.requires_grad_(False)


def _load_exposure(model_data: Dict[str, Any]) -> Optional[Module]:
    """the checkpoint's per-image exposure compensation, frozen (None: the checkpoint has none -- every reference checkpoint)"""
    if EXPOSURE not in model_data:
        return None
    from thre3d_atom.thre3d_reprs.exposure import PerImageExposure

    exposure = PerImageExposure(**model_data[EXPOSURE][CONFIG_DICT])
    exposure.load_state_dict(model_data[EXPOSURE][STATE_DICT])
    return exposure.requires_grad_(False)


def create_volumetric_model_from_saved_model(
    model_path: Path,
    thre3d_repr_creator: Callable[[Dict[str, Any]], Module],
    device: torch.device = torch.device("cpu"),
) -> Tuple[VolumetricModel, Dict[str, Any]]:
    return _load_model(model_path, thre3d_repr_creator, device)


def create_volumetric_model_from_saved_model_attn(
    model_path: Path,
    thre3d_repr_creator: Callable[..., Module],
    device: torch.device = torch.device("cpu"),
    load_attn=False,
) -> Tuple[VolumetricModel, Dict[str, Any]]:
    return _load_model(model_path, lambda data: thre3d_repr_creator(data, load_attn=load_attn), device)
