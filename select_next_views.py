#!/usr/bin/env python3
"""Rank candidate cameras of a trained voxel grid by expected information gain (next-best-view selection).

The per-voxel Fisher information H of the rendered colours with respect to the densities is accumulated over the training
cameras of -d; every candidate is scored by sum_v H_candidate[v] / (H[v] + prior_precision), the best one is taken, its own
information is added to H, and the others are scored again: --num_select greedy rounds.  Candidates come from --candidates (a
file in the `<split>_camera_params.json` schema) or from --num_candidates poses of the checkpoint's 360 degree path.  Writes
next_views.json (the ranked candidates, their gains before and after each round, the poses in the dataset's schema) and
fisher.pth (H of the training set); --uncertainty_maps adds uncertainty_NNNN.png per selected view, the log-scaled predictive
variance next to the colour render.  Both passes run on the GPU (vox-e_amd/csrc/voxe_fisher.hip)."""
import json
import os
import sys
from pathlib import Path

import click
import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.data.constants import BOUNDS, EXTRINSIC, INTRINSIC, ROTATION, TRANSLATION  # noqa: E402
from thre3d_atom.data.datasets import camera_to_params  # noqa: E402
from thre3d_atom.modules.volumetric_model import create_volumetric_model_from_saved_model  # noqa: E402
from thre3d_atom.thre3d_reprs import fisher as F  # noqa: E402
from thre3d_atom.thre3d_reprs.visibility import visibility_cameras  # noqa: E402
from thre3d_atom.thre3d_reprs.voxels import create_voxel_grid_from_saved_info_dict  # noqa: E402
from thre3d_atom.utils.constants import HEMISPHERICAL_RADIUS  # noqa: E402
from thre3d_atom.utils.imaging_utils import CameraPose, get_thre360_animation_poses, to8b  # noqa: E402


def candidates_from_file(path: Path):
    """(names, poses) of a `<split>_camera_params.json`-schema file, in the file's order"""
    params = json.loads(Path(path).read_text())
    names = list(params)
    return names, [CameraPose(np.array(params[n][EXTRINSIC][ROTATION], dtype=np.float32).reshape(3, 3),
                              np.array(params[n][EXTRINSIC][TRANSLATION], dtype=np.float32).reshape(3, 1)) for n in names]


def pose_entry(pose: CameraPose, intrinsics, bounds) -> dict:
    """one camera in the dataset's schema"""
    intr = camera_to_params(intrinsics)
    intr[BOUNDS] = [float(bounds[0]), float(bounds[1])]
    return {EXTRINSIC: {ROTATION: np.asarray(torch.as_tensor(pose.rotation).cpu(), dtype=np.float64).reshape(3, 3).tolist(),
                        TRANSLATION: np.asarray(torch.as_tensor(pose.translation).cpu(), dtype=np.float64).reshape(3, 1).tolist()},
            INTRINSIC: intr}


def heat_map(var: np.ndarray) -> np.ndarray:
    """[H,W,3] uint8 of log10(var) between its 1st and 99th percentile over the pixels that hit the grid (black: var == 0):
    dark blue (certain) -> yellow (uncertain)"""
    out = np.zeros(var.shape + (3,), dtype=np.float32)
    hit = var > 0
    if hit.any():
        lv = np.log10(var[hit])
        lo, hi = np.percentile(lv, 1.0), np.percentile(lv, 99.0)
        t = np.clip((lv - lo) / max(hi - lo, 1e-12), 0.0, 1.0)
        out[hit] = np.stack([t, t * t * 0.9 + 0.05, 0.6 * (1.0 - t) + 0.1], axis=-1)
    return to8b(out)


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="path to the trained / edited / refined model")
@click.option("-d", "--data_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="dataset whose training cameras are the photographs already taken")
@click.option("-o", "--output_path", type=click.Path(file_okay=False, dir_okay=True), required=True, help="directory for next_views.json, fisher.pth and the maps")
@click.option("--candidates", type=click.Path(file_okay=True, dir_okay=False), default=None, help="candidate cameras, a <split>_camera_params.json-schema file (default: the 360 degree path)")
@click.option("--num_candidates", type=click.IntRange(min=1), default=72, show_default=True, help="poses of the 360 degree path (without --candidates)")
@click.option("--camera_pitch", type=click.FLOAT, default=60.0, show_default=True, help="pitch of the 360 degree path")
@click.option("--num_select", type=click.IntRange(min=1), default=5, show_default=True, help="greedy rounds: views to select")
@click.option("--prior_precision", type=click.FLOAT, default=None, help="lambda of 1 / (H + lambda) (default: 1e-6 x the training set's largest H, an untuned guard)")
@click.option("--uncertainty_maps", is_flag=True, default=False, help="also write uncertainty_NNNN.png per selected view: log-scaled variance | colour render")
@click.option("--overridden_num_samples_per_ray", type=click.IntRange(min=1), default=None, help="samples per ray (default: the model's)")
def main(**kwargs) -> None:
    cfg = type("Config", (), kwargs)
    device = torch.device("cuda")
    out = Path(cfg.output_path)
    out.mkdir(exist_ok=True, parents=True)
    vol_mod, extra = create_volumetric_model_from_saved_model(Path(cfg.model_path), create_voxel_grid_from_saved_info_dict, device=device)
    train_poses, intrinsics = visibility_cameras(extra, cfg.data_path)
    if cfg.candidates is not None:
        names, cand_poses = candidates_from_file(Path(cfg.candidates))
        source = str(cfg.candidates)
    else:
        # (num_candidates poses: get_thre360_animation_poses drops the closing duplicate of its linspace)
        cand_poses = list(get_thre360_animation_poses(extra[HEMISPHERICAL_RADIUS], cfg.camera_pitch, cfg.num_candidates + 1))
        names = [f"thre360_{n:04d}" for n in range(len(cand_poses))]
        source = f"thre360 path: {len(cand_poses)} poses, pitch {cfg.camera_pitch}"
    overrides = {}
    if cfg.overridden_num_samples_per_ray is not None:
        overrides["num_samples_per_ray"] = int(cfg.overridden_num_samples_per_ray)
    fisher = F.accumulate_fisher(vol_mod, train_poses, intrinsics, **overrides)
    lam = cfg.prior_precision if cfg.prior_precision is not None else F.default_prior_precision(fisher)
    sel = F.select_next_views(vol_mod, train_poses, cand_poses, intrinsics, cfg.num_select, lam, train_fisher=fisher, **overrides)
    torch.save({"fisher": fisher.cpu(), "prior_precision": float(lam), "num_train_views": len(train_poses)}, out / "fisher.pth")
    bounds = vol_mod.render_config.camera_bounds
    report = {
        "model": str(cfg.model_path), "num_train_views": len(train_poses), "candidates": source, "num_candidates": len(cand_poses),
        "prior_precision": float(lam),
        "selected": [dict(rank=n, candidate=int(i), name=names[i], gain=float(g), gain_after=float(a),
                          **pose_entry(cand_poses[i], intrinsics, bounds))
                     for n, (i, g, a) in enumerate(zip(sel.indices, sel.gains, sel.gains_after))],
        # gains of every candidate before each round (null: already selected)
        "rounds": [dict(round=n, selected=int(sel.indices[n]), gains=[None if g != g else float(g) for g in gains])
                   for n, gains in enumerate(sel.rounds)],
    }
    (out / "next_views.json").write_text(json.dumps(report, indent=1))
    if cfg.uncertainty_maps:
        from PIL import Image

        for n, i in enumerate(sel.indices):
            var = F.uncertainty_map(vol_mod, cand_poses[i], intrinsics, fisher, lam, **overrides).cpu().numpy()
            colour = vol_mod.render(cand_poses[i], intrinsics, gpu_render=True, **overrides).colour.cpu().numpy()
            Image.fromarray(np.concatenate([heat_map(var), to8b(colour)], axis=1)).save(out / f"uncertainty_{n:04d}.png")
    print(f"{len(train_poses)} training views, {len(cand_poses)} candidates, prior precision {lam:.3e}: selected "
          + ", ".join(f"{names[i]} (gain {g:.4g})" for i, g in zip(sel.indices, sel.gains)) + f"  -> {out / 'next_views.json'}")


if __name__ == "__main__":
    main()
