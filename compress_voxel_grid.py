#!/usr/bin/env python3
"""Compress a trained, edited or refined voxel grid for storage: voxels are scored by the rendering weight they receive over a
set of cameras, the ones that carry the last --prune_share of that mass are dropped, the ones that carry the first --keep_share
are stored exactly (float16 by default) and the features of the rest are vector-quantised against a codebook of
--codebook_size entries trained by weighted k-means (VQRF, Li et al., CVPR 2023).  The output is a checkpoint the loaders of the
render, test, mesh-export and view-selection tools read directly; decompress_voxel_grid.py turns it back into an ordinary one.
The cameras are the training split of -d, or --num_views poses of the checkpoint's own 360 degree animation path.  The
importance pass and the k-means run on the GPU (vox-e_amd/csrc/voxe_lift.hip, voxe_vq.hip)."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs import compression as CP  # noqa: E402
from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_DENSITIES, u_FEATURES  # noqa: E402
from thre3d_atom.thre3d_reprs.visibility import visibility_cameras  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402


def render_psnr(a, b) -> float:
    """PSNR (dB, peak 1) of two colour renders"""
    mse = float(((a.to(torch.float64) - b.to(torch.float64)) ** 2).mean())
    return float("inf") if mse == 0.0 else -10.0 * float(torch.log10(torch.tensor(mse, dtype=torch.float64)))


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="compressed checkpoint (.pth)")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), default=None, help="dataset whose training cameras are used")
@click.option("--num_views", type=click.IntRange(min=1), default=36, show_default=True, help="poses of the 360 degree path (without -d)")
@click.option("--prune_share", type=click.FloatRange(0.0, 1.0), default=CP.DEFAULT_PRUNE_SHARE, show_default=True, help="share of the importance mass whose voxels are dropped")
@click.option("--keep_share", type=click.FloatRange(0.0, 1.0), default=CP.DEFAULT_KEEP_SHARE, show_default=True, help="share of the importance mass whose voxels are stored exactly")
@click.option("--codebook_size", type=click.IntRange(1, 65536), default=CP.DEFAULT_CODEBOOK_SIZE, show_default=True, help="codewords of the vector quantiser")
@click.option("--kmeans_iterations", type=click.IntRange(min=0), default=CP.DEFAULT_ITERATIONS, show_default=True, help="Lloyd iterations")
@click.option("--store_dtype", type=click.Choice(["float16", "float32"]), default="float16", show_default=True, help="precision of the values stored exactly")
@click.option("--seed", type=click.INT, default=0, show_default=True, help="seed of the codebook initialisation")
@click.option("--overridden_num_samples_per_ray", type=click.IntRange(min=1), default=None, help="samples per ray (default: the model's)")
@click.option("--evaluate", is_flag=True, default=False, help="also print the PSNR of the decompressed model's renders against the original's")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    path = Path(cfg.model_path)
    data = CP.load_uncompressed_checkpoint(path)
    if CP.u_ATTN in data[THRE3D_REPR][STATE_DICT]:
        raise click.UsageError(f"{path} carries attention parameters (a keep grid): such checkpoints cannot be compressed")
    vol_mod, extra = create_volumetric_model_from_saved_model(path, create_voxel_grid_from_saved_info_dict, device=device)
    poses, intrinsics = visibility_cameras(extra, cfg.data_path, cfg.num_views)
    overrides = {}
    if cfg.overridden_num_samples_per_ray is not None:
        overrides["num_samples_per_ray"] = int(cfg.overridden_num_samples_per_ray)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    importance = CP.voxel_importance(vol_mod, poses, intrinsics, **overrides)
    ev[1].record()
    compressed = CP.compress(vol_mod, importance, cfg.prune_share, cfg.keep_share, cfg.codebook_size, cfg.kmeans_iterations,
                             cfg.store_dtype, cfg.seed)
    ev[2].record()
    torch.cuda.synchronize()
    state = data[THRE3D_REPR][STATE_DICT]
    grid_bytes = sum(state[k].numel() * state[k].element_size() for k in (u_DENSITIES, u_FEATURES))
    before = CP.checkpoint_bytes(data)
    out = Path(cfg.output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    CP.save_compressed(out, data, compressed)
    after = out.stat().st_size
    labels = compressed.labels()
    counts = [int((labels == v).sum()) for v in (CP.LABEL_PRUNED, CP.LABEL_VQ, CP.LABEL_KEPT)]
    print(f"{len(poses)} views: {labels.size} voxels: pruned {counts[0]}  vector-quantised {counts[1]}  kept {counts[2]}  "
          f"codebook {compressed.codebook.shape[0]} x {compressed.codebook.shape[1]}")
    print(f"bytes: {before} before ({grid_bytes} in the grid tensors)  {after} after  ratio {before / max(after, 1):.2f}")
    print("distortion per iteration: " + " ".join(f"{v:.6e}" for v in compressed.distortion))
    print(f"importance {ev[0].elapsed_time(ev[1]):.2f} ms  partition + k-means {ev[1].elapsed_time(ev[2]):.2f} ms  -> {out}")
    if cfg.evaluate:
        small, _ = create_volumetric_model_from_saved_model(out, create_voxel_grid_from_saved_info_dict, device=device)
        kw = dict(perturb_sampled_points=False, **overrides)
        values = []
        for pose in poses:
            a, b = vol_mod.render(pose, intrinsics, **kw).colour, small.render(pose, intrinsics, **kw).colour
            values.append(render_psnr(a, b))
        finite = [v for v in values if v != float("inf")]
        mean = sum(finite) / len(finite) if finite else float("inf")
        print(f"evaluate: PSNR of the decompressed model against the original over {len(poses)} views: "
              f"mean {mean:.2f} dB  min {min(values):.2f} dB")


if __name__ == "__main__":
    main()
