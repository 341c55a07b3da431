"""Held-out evaluation of a trained model (interface of the reference's thre3d_atom/modules/testers.py:17-71).

Every test view is one fused HIP forward launch (`optimized_sampling=True`, `render_num_samples_per_ray` samples, like
the reference); PSNR and SSIM (voxe_hip.ops.ssim; not in the reference) are computed on the GPU, and so are
their colour-corrected forms (voxe_hip.ops.fit_affine_colour; not in the reference) for captures whose images
differ in exposure.  LPIPS needs the external `lpips` network: it is reported when that
package is importable and skipped otherwise (the reference hard-requires it)."""
from typing import Any, Dict, Optional

import numpy as np
import torch
from torch.nn.functional import mse_loss

from thre3d_atom.modules.volumetric_model import VolumetricModel
from thre3d_atom.utils.imaging_utils import CameraPose
from thre3d_atom.utils.logging import log
from thre3d_atom.utils.metric_utils import SSIM_MIN_SIDE, mse2psnr, ssim
from voxe_hip.ops import fit_affine_colour


def test_sh_vox_grid_vol_mod_with_posed_images(
    vol_mod: VolumetricModel,
    test_dl: Any,                       # DataLoader (batch size 1) or a posed-images dataset
    parallel_rays_chunk_size: Optional[int] = None,
    tensorboard_writer: Any = None,
    global_step: Optional[int] = None,
    colour_corrected: bool = False,     # addition of this build: also report "cc_psnr" (and "cc_ssim"): each render is fitted to
                                        # its image by a least-squares affine colour transform before it is scored (mip-NeRF 360,
                                        # RawNeRF).  A model with exposure compensation reports them either way
) -> Dict[str, float]:
    dataset = getattr(test_dl, "dataset", test_dl)
    intrinsics = dataset.camera_intrinsics
    log.info(f"Testing the model on {len(dataset)} heldout images")
    lpips_net = None
    try:
        import lpips  # noqa: WPS433 (optional dependency)

        lpips_net = lpips.LPIPS(net="vgg").to(vol_mod.device)
    except ImportError:
        pass
    colour_corrected = bool(colour_corrected) or vol_mod.exposure is not None
    psnrs, lpipss, ssims, cc_psnrs, cc_ssims = [], [], [], [], []
    for index in range(len(dataset)):
        image, pose, _ = dataset[index]
        image, pose = image.to(vol_mod.device), pose
        rendered = vol_mod.render(
            camera_pose=CameraPose(rotation=pose[:, :3], translation=pose[:, 3:]), camera_intrinsics=intrinsics,
            parallel_rays_chunk_size=parallel_rays_chunk_size, gpu_render=True, optimized_sampling=True,
            num_samples_per_ray=vol_mod.render_config.render_num_samples_per_ray)
        colour = rendered.colour.permute(2, 0, 1)
        with torch.no_grad():
            psnrs.append(float(mse2psnr(mse_loss(colour, image).item())))
            if min(colour.shape[1:]) >= SSIM_MIN_SIDE:   # smaller views have no 11 x 11 window: skipped for this key
                ssims.append(ssim(rendered.colour, image.permute(1, 2, 0)))
            if colour_corrected:
                if image.shape[0] != 3 or rendered.colour.shape[-1] != 3:
                    raise ValueError(f"the colour-corrected metrics fit a 3 x 4 affine: they need images of 3 channels; got "
                                     f"{image.shape[0]} (render: {rendered.colour.shape[-1]})")
                # (the render itself is never altered: the fitted copy is scored and dropped)
                flat, target = rendered.colour.reshape(1, -1, 3), image.permute(1, 2, 0).reshape(1, -1, 3)
                A, b = fit_affine_colour(flat, target)
                fitted = (flat[0] @ A[0].float().T + b[0].float()).reshape(rendered.colour.shape)
                cc_psnrs.append(float(mse2psnr(mse_loss(fitted, image.permute(1, 2, 0)).item())))
                if min(colour.shape[1:]) >= SSIM_MIN_SIDE:
                    cc_ssims.append(ssim(fitted, image.permute(1, 2, 0)))
            if lpips_net is not None:
                lpipss.append(float(lpips_net(colour[None], image[None], normalize=True).item()))
    out = {"psnr": float(np.mean(psnrs))}
    log.info(f"Mean PSNR on holdout set: {out['psnr']}")
    if ssims:
        out["ssim"] = float(np.mean(ssims))
        log.info(f"Mean SSIM on holdout set: {out['ssim']}")
    if cc_psnrs:
        out["cc_psnr"] = float(np.mean(cc_psnrs))
        log.info(f"Mean colour-corrected PSNR on holdout set: {out['cc_psnr']}")
    if cc_ssims:
        out["cc_ssim"] = float(np.mean(cc_ssims))
        log.info(f"Mean colour-corrected SSIM on holdout set: {out['cc_ssim']}")
    if lpipss:
        out["lpips"] = float(np.mean(lpipss))
        log.info(f"Mean LPIPS on holdout set: {out['lpips']}")
    if tensorboard_writer is not None and global_step is not None:
        tensorboard_writer.add_scalar("TEST_SET_PSNR", out["psnr"], global_step=global_step)
        if "ssim" in out:
            tensorboard_writer.add_scalar("TEST_SET_SSIM", out["ssim"], global_step=global_step)
        for key in ("cc_psnr", "cc_ssim"):
            if key in out:
                tensorboard_writer.add_scalar(f"TEST_SET_{key.upper()}", out[key], global_step=global_step)
        if "lpips" in out:
            tensorboard_writer.add_scalar("TEST_SET_LPIPS", out["lpips"], global_step=global_step)
    return out


test_sh_vox_grid_vol_mod_with_posed_images.__test__ = False  # a library function whose reference name starts with "test_"
