#!/usr/bin/env python3
"""Turn a checkpoint written by compress_voxel_grid.py back into an ordinary one: the density and feature tensors are rebuilt
(pruned voxels at the field's empty density with zero features, vector-quantised voxels from the codebook, the rest from the
stored values) and every other entry of the file is written back untouched.  Runs on the host."""
import os
import sys
from pathlib import Path

import click
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "vox-e_amd"))

from thre3d_atom.thre3d_reprs import compression as CP  # noqa: E402


@click.command()
@click.option("-i", "--model_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="compressed checkpoint")
@click.option("-o", "--output_path", type=click.Path(file_okay=True, dir_okay=False), required=True, help="ordinary checkpoint (.pth)")
def main(model_path, output_path) -> None:
    data = torch.load(Path(model_path), map_location="cpu", weights_only=False)
    if not CP.expand_checkpoint_(data):
        raise click.UsageError(f"{model_path} holds no compressed voxel grid: there is nothing to decompress")
    out = Path(output_path)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save(data, out)
    print(f"{model_path} ({Path(model_path).stat().st_size} bytes) -> {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
