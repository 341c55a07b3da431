#!/usr/bin/env python3
"""nerfstudio transforms.json -> `<split>_camera_params.json` of this project, with the camera's fl_x, fl_y, cx, cy and
k1, k2, p1, p2 (k3 when present).

    python tools/convert_from_nerfstudio_transforms.py -t transforms.json -o scene --near 0.5 --far 6 [--split train] [--recentre]

The intrinsics must be given once for the whole file (w, h, fl_x, fl_y, cx, cy at the top level): per-frame intrinsics are not
supported (one shared camera per dataset); a fisheye `camera_model` is out of scope.  `transform_matrix` is already an OpenGL
camera-to-world matrix (x right, y up, looking down -z), which is this project's convention.  Entries are keyed by the image's
file name.  Standard library + numpy only."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_import as CI  # noqa: E402

INTRINSICS = ("w", "h", "fl_x", "fl_y", "cx", "cy")
SUPPORTED_MODELS = ("OPENCV", "PINHOLE", "SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


class UnsupportedModel(ValueError):
    pass


def convert(transforms_path, near, far, recentre=False):
    meta = json.loads(Path(transforms_path).read_text())
    model = str(meta.get("camera_model", "OPENCV")).upper()
    if model not in SUPPORTED_MODELS:
        raise UnsupportedModel(f"camera_model {model} is not supported (supported: {', '.join(SUPPORTED_MODELS)}); fisheye / "
                               f"equidistant models are out of scope")
    missing = [k for k in INTRINSICS if k not in meta]
    if missing:
        raise UnsupportedModel(f"{transforms_path} has no top-level {missing}: per-frame intrinsics are not supported (one shared "
                               f"camera per dataset)")
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError(f"{transforms_path} lists no frame")
    for frame in frames:
        clash = [k for k in INTRINSICS if k in frame and float(frame[k]) != float(meta[k])]
        if clash:
            raise UnsupportedModel(f"frame {frame.get('file_path')} overrides {clash}: per-frame intrinsics are not supported")
    dist = [float(meta.get(k, 0.0)) for k in ("k1", "k2", "p1", "p2", "k3")]
    mats = [np.asarray(f["transform_matrix"], np.float64)[:3, :4] for f in frames]
    shift = CI.optical_axes_meeting_point([m[:, :3] for m in mats], [m[:, 3] for m in mats]) if recentre else np.zeros(3)
    entries = {}
    for frame, m in zip(frames, mats):
        entries[Path(frame["file_path"]).name] = CI.entry(meta["h"], meta["w"], meta["fl_x"], meta["fl_y"], meta["cx"], meta["cy"],
                                                          dist, m[:, :3], m[:, 3] - shift, near, far)
    return dict(sorted(entries.items()))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-t", "--transforms", required=True, help="path to transforms.json")
    ap.add_argument("-o", "--output_path", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--near", type=float, required=True)
    ap.add_argument("--far", type=float, required=True)
    ap.add_argument("--recentre", action="store_true")
    args = ap.parse_args(argv)
    try:
        entries = convert(args.transforms, args.near, args.far, args.recentre)
    except UnsupportedModel as e:
        print(f"convert_from_nerfstudio_transforms: unsupported: {e}", file=sys.stderr)
        return 2
    path = CI.write_params(args.output_path, args.split, entries)
    print(f"{len(entries)} cameras -> {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
