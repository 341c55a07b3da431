"""Checkpoint compression of a VoxelGrid: importance pruning and vector quantisation (DESIGN.md section 4.25 "Compression";
VQRF, Li et al., CVPR 2023).  Not in the reference.

    importance   I[v] = sum over (cameras, rays, samples) of w_k t_c: the rendering weight a voxel ever receives -- sum_w of
                 voxe_lift_accumulate in coverage-only mode, 64-bit fixed point, bit-reproducible
    partition    voxels sorted by (importance descending, linear index ascending), P_i their inclusive prefix sums:
                     kept exactly (2)  iff  P_i - I_i <  t_keep  = int(keep_share * float(total))
                     pruned (0)        iff  I_i == 0  or  P_i - I_i >= t_prune = int((1 - prune_share) * float(total))
                     vector-quantised (1) otherwise;  where both tests hold (prune_share + keep_share > 1) pruned wins
    codebook     weighted k-means (Lloyd) over the features of the VQ voxels: voxe_vq_assign on the matrix cores and
                 voxe_vq_accumulate in fixed point (voxe_vq.hip), so a seed gives one codebook, bit for bit
    container    two bit-packed masks, densities of the non-pruned voxels and features of the kept ones in float16 (or
                 float32), uint16 codebook indices, a float32 codebook; in a file every array is zlib-deflated

Nothing here is differentiable; joint fine-tuning after quantisation (VQRF's last stage) is not part of this module."""
import dataclasses
import zlib
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from thre3d_atom.thre3d_reprs.constants import STATE_DICT, THRE3D_REPR, u_ATTN, u_DENSITIES, u_FEATURES

COMPRESSED = "compressed"            # the checkpoint entry (under THRE3D_REPR) that stands for the two grid tensors
LABEL_PRUNED, LABEL_VQ, LABEL_KEPT = 0, 1, 2
DEFAULT_PRUNE_SHARE, DEFAULT_KEEP_SHARE, DEFAULT_CODEBOOK_SIZE = 1e-3, 0.6, 4096    # VQRF's
DEFAULT_ITERATIONS = 10              # DESIGN.md 4.25 holds the distortion curve behind it
DECOMPRESS_TOOL = "decompress_voxel_grid.py"
_ONE = float(1 << 32)                # the fixed-point unit of the importance and of the centroid sums
_TOTAL_LIMIT = 1 << 62
_STORE_DTYPES = {"float16": np.float16, "float32": np.float32}


# ---- importance -----------------------------------------------------------------------------------------------------------------
def voxel_importance(vol_mod, poses: Sequence, camera_intrinsics, **render_overrides) -> Tensor:
    """int64 [X,Y,Z]: sum_w of voxe_lift_accumulate in coverage-only mode over `poses`, the rays cast and the render parameters
    chosen exactly as lifting.lift_images does (stratified jitter off unless perturb_sampled_points=True is passed): the same
    bits as lift_images(...).sum_w for the same cameras."""
    from thre3d_atom.rendering.volumetric.utils.misc import cast_rays, flatten_rays
    from thre3d_atom.thre3d_reprs.renderers import _render_params
    from voxe_hip import ops as _ops

    grid = vol_mod.thre3d_repr
    overrides = {"perturb_sampled_points": False, **render_overrides}
    config = vol_mod._update_render_config(vol_mod.render_config, overrides)
    spec = grid.voxe_grid_spec(attn=False)
    dens = grid.densities.detach()
    sum_w = torch.zeros(dens.shape[:3], dtype=torch.int64, device=dens.device)
    for pose in poses:
        rays = flatten_rays(cast_rays(camera_intrinsics, pose, device=vol_mod.device))
        params = _render_params(grid, rays, config, attn=False)
        _ops.lift_accumulate_(spec, params, dens, rays.origins, rays.directions, None, None, sum_w)
    return sum_w


# ---- partition ------------------------------------------------------------------------------------------------------------------
def partition_thresholds(total: int, prune_share: float, keep_share: float) -> Tuple[int, int]:
    """(t_keep, t_prune) for an importance total (a python int)"""
    if not (0.0 <= prune_share <= 1.0 and 0.0 <= keep_share <= 1.0):
        raise ValueError(f"prune_share and keep_share must lie in [0, 1]; got {prune_share}, {keep_share}")
    if not 0 <= total < _TOTAL_LIMIT:
        raise ValueError(f"the importance total {total} is outside 0 .. 2^62 - 1")
    return int(keep_share * float(total)), int((1.0 - prune_share) * float(total))


def partition(importance: Tensor, prune_share: float = DEFAULT_PRUNE_SHARE, keep_share: float = DEFAULT_KEEP_SHARE) -> Tensor:
    """uint8 labels of importance's shape: 0 pruned, 1 vector-quantised, 2 kept exactly (the rule of the module docstring).
    Integer arithmetic throughout: int64 prefix sums, thresholds from python ints; runs on importance's device."""
    flat = importance.reshape(-1)
    if flat.dtype != torch.int64:
        raise ValueError(f"importance must be int64 (32 fraction bits); got {flat.dtype}")
    if flat.numel() and int(flat.min()) < 0:
        raise ValueError("importance must be non-negative")
    # (a float64 bound first: the int64 sum of values that overflow it would wrap)
    if float(flat.to(torch.float64).sum()) >= float(_TOTAL_LIMIT):
        raise ValueError("the importance total is 2^62 or more")
    total = int(flat.sum())
    t_keep, t_prune = partition_thresholds(total, float(prune_share), float(keep_share))
    ordered, order = torch.sort(flat, descending=True, stable=True)     # stable: ties stay in ascending linear index
    before = torch.cumsum(ordered, 0) - ordered
    lab = torch.full_like(ordered, LABEL_VQ, dtype=torch.uint8)
    lab[before < t_keep] = LABEL_KEPT
    lab[(ordered == 0) | (before >= t_prune)] = LABEL_PRUNED
    labels = torch.empty_like(lab)
    labels[order] = lab
    return labels.reshape(importance.shape)


# ---- codebook -------------------------------------------------------------------------------------------------------------------
def lloyd_update(codebook: Tensor, sum_wx: Tensor, sum_w: Tensor) -> Tensor:
    """the codebook after one Lloyd step: float32(sum_wx / sum_w), divided in float64; a codeword with sum_w == 0 keeps its
    value"""
    mean = (sum_wx.to(torch.float64) / sum_w.to(torch.float64).clamp(min=1.0)[:, None]).to(torch.float32)
    return torch.where((sum_w != 0)[:, None], mean, codebook)


def train_codebook(features: Tensor, weights: Tensor, codebook_size: int, iterations: int,
                   seed: int = 0) -> Tuple[Tensor, Tensor, List[float]]:
    """Weighted k-means over `features` ([N,F] float32 on the GPU, F in 1..64) with `weights` ([N], >= 0).  Both are normalised
    once in float32 (x / max|x|, w / max w); the codebook starts from K distinct rows, torch.randperm(N) of a CPU generator
    seeded with `seed` (every row its own codeword when N <= K); then `iterations` Lloyd steps of ops.vq_assign_ and
    ops.vq_accumulate_, each followed by lloyd_update, and one last assignment against the final codebook.
    Returns (codebook [K',F] float32 scaled back by max|x|, K' = min(K, N); index [N] int32 into it; the weighted distortion
    sum_n w~_n dist_n of the normalised data under each iteration's assignment, iterations + 1 values)."""
    from voxe_hip import ops as _ops

    if features.dim() != 2 or weights.shape != features.shape[:1]:
        raise ValueError(f"features must be [N,F] and weights [N]; got {tuple(features.shape)}, {tuple(weights.shape)}")
    N, F = (int(v) for v in features.shape)
    K = min(int(codebook_size), N)
    if not 1 <= int(codebook_size) <= 65536:
        raise ValueError(f"codebook_size must lie in 1..65536; got {codebook_size}")
    device = features.device
    if N == 0:
        return (torch.zeros((0, F), dtype=torch.float32, device=device), torch.zeros((0,), dtype=torch.int32, device=device), [])
    x = features.detach().to(torch.float32).contiguous()
    w = weights.detach().to(torch.float32).contiguous()
    x_scale, w_scale = float(x.abs().max()), float(w.max())
    x_scale = x_scale if x_scale > 0.0 else 1.0
    w_scale = w_scale if w_scale > 0.0 else 1.0
    x = x / torch.tensor(x_scale, dtype=torch.float32, device=device)
    w = w / torch.tensor(w_scale, dtype=torch.float32, device=device)
    if N <= int(codebook_size):
        rows = torch.arange(N)
    else:
        rows = torch.randperm(N, generator=torch.Generator(device="cpu").manual_seed(int(seed)))[:K]
    codebook = x[rows.to(device)].contiguous()
    index = torch.empty((N,), dtype=torch.int32, device=device)
    dist = torch.empty((N,), dtype=torch.float32, device=device)
    sum_wx = torch.empty((K, F), dtype=torch.int64, device=device)
    sum_w = torch.empty((K,), dtype=torch.int64, device=device)
    curve = []
    for it in range(int(iterations) + 1):
        _ops.vq_assign_(x, codebook, index, dist)
        curve.append((w.to(torch.float64) * dist.to(torch.float64)).sum())
        if it == int(iterations):
            break
        sum_wx.zero_()
        sum_w.zero_()
        # points sorted by codeword: the kernel's shipped variant then merges each run inside the wave and issues one atomic
        # per run and channel (8 x faster than atomics on the points as they come, sort and gather included
        # 4 x); the sums are integers, so the order changes no bit.  (vq_assign_ wrote the index: it is in range)
        by_code, order = torch.sort(index)
        _ops.vq_accumulate_(x[order], w[order], by_code, sum_wx, sum_w, check_index=False)
        codebook = lloyd_update(codebook, sum_wx, sum_w).contiguous()
    return codebook * torch.tensor(x_scale, dtype=torch.float32, device=device), index, [float(v) for v in curve]


# ---- the container --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class CompressedGrid:
    dims: Tuple[int, int, int]
    feature_dims: int
    pruned_bits: np.ndarray       # uint8, np.packbits of (labels == 0) over the linear voxel index
    kept_bits: np.ndarray         # uint8, np.packbits of (labels == 2)
    densities: np.ndarray         # store dtype [non-pruned voxels], ascending linear index
    kept_features: np.ndarray     # store dtype [kept voxels, F], ascending linear index
    indices: np.ndarray           # uint16 [VQ voxels], ascending linear index
    codebook: np.ndarray          # float32 [K, F]
    empty_density: float          # what a pruned voxel's raw density decompresses to
    dtypes: Tuple[str, str]       # torch dtypes of the checkpoint's density and feature tensors, by name
    distortion: Tuple[float, ...] = ()   # the k-means curve (information only)

    ARRAYS = ("pruned_bits", "kept_bits", "densities", "kept_features", "indices", "codebook")

    def labels(self) -> np.ndarray:
        """uint8 [X,Y,Z]"""
        n = int(np.prod(self.dims))
        pruned = np.unpackbits(self.pruned_bits, count=n).astype(bool)
        kept = np.unpackbits(self.kept_bits, count=n).astype(bool)
        lab = np.full(n, LABEL_VQ, dtype=np.uint8)
        lab[kept] = LABEL_KEPT
        lab[pruned] = LABEL_PRUNED
        return lab.reshape(self.dims)

    def nbytes(self) -> int:
        """bytes of the arrays before deflation"""
        return sum(int(getattr(self, name).nbytes) for name in self.ARRAYS)


def _empty_density_of(grid) -> float:
    from thre3d_atom.thre3d_reprs.visibility import empty_raw_density
    from thre3d_atom.thre3d_reprs.voxels import density_activation_codes

    pre, post = density_activation_codes(grid._density_preactivation, grid._density_postactivation)
    return empty_raw_density(pre, post, float(grid._expected_density_scale))


def _stored(values: Tensor, store_dtype, what: str) -> np.ndarray:
    arr = values.detach().to(device="cpu", dtype=torch.float32).numpy()
    if not np.isfinite(arr).all():
        raise ValueError(f"{what} hold values that are not finite")
    if store_dtype == np.float16 and arr.size and float(np.abs(arr).max()) > float(np.finfo(np.float16).max):
        raise ValueError(f"{what} hold |value| {float(np.abs(arr).max()):.6g}, beyond float16's range "
                         f"({float(np.finfo(np.float16).max):.0f}): store with float32")
    return arr.astype(store_dtype)


def compress(vol_mod, importance: Tensor, prune_share: float = DEFAULT_PRUNE_SHARE, keep_share: float = DEFAULT_KEEP_SHARE,
             codebook_size: int = DEFAULT_CODEBOOK_SIZE, iterations: int = DEFAULT_ITERATIONS, store_dtype="float16",
             seed: int = 0) -> CompressedGrid:
    """Compress the VoxelGrid of `vol_mod` given its importance grid (voxel_importance): partition, k-means over the features
    of the VQ voxels weighted by their importance, and the container.  codebook_size in 1..65536 (uint16 indices).  ValueError
    for a grid with attention parameters, for one without an empty density value and for values beyond float16's range."""
    grid = vol_mod.thre3d_repr
    if getattr(grid, "attn", None) is not None:
        raise ValueError("a grid that carries attention parameters cannot be compressed")
    store = _STORE_DTYPES[store_dtype if isinstance(store_dtype, str) else str(store_dtype).replace("torch.", "")]
    dens, feat = grid.densities.detach(), grid.features.detach()
    dims = tuple(int(v) for v in dens.shape[:3])
    if tuple(importance.shape) != dims:
        raise ValueError(f"importance must be [X,Y,Z]={dims}; got {tuple(importance.shape)}")
    empty = _empty_density_of(grid)
    labels = partition(importance.to(dens.device), prune_share, keep_share)
    vq = labels.reshape(-1) == LABEL_VQ
    weights = (importance.to(dens.device).reshape(-1)[vq].to(torch.float64) / _ONE).to(torch.float32)
    features = feat.reshape(-1, feat.shape[-1])[vq].to(torch.float32)
    codebook, index, curve = train_codebook(features, weights, codebook_size, iterations, seed)
    return build_container(labels, dens, feat, index, codebook, empty, store, curve)


def build_container(labels: Tensor, densities: Tensor, features: Tensor, index: Tensor, codebook: Tensor, empty_density: float,
                    store_dtype=np.float16, distortion: Sequence[float] = ()) -> CompressedGrid:
    """The container of a grid ([X,Y,Z,1] densities, [X,Y,Z,F] features) given its labels ([X,Y,Z] uint8), the codebook
    ([K,F], K <= 65536) and the codeword index of every VQ voxel in ascending linear voxel index"""
    dims = tuple(int(v) for v in densities.shape[:3])
    F = int(features.shape[-1])
    labels = labels.reshape(-1).to(densities.device)
    if int(codebook.shape[0]) > 65536 or index.numel() != int((labels == LABEL_VQ).sum()):
        raise ValueError("the codebook has more than 65536 entries or the indices do not match the vector-quantised voxels")
    kept = labels == LABEL_KEPT
    return CompressedGrid(
        dims=dims, feature_dims=F,
        pruned_bits=np.packbits((labels == LABEL_PRUNED).cpu().numpy()), kept_bits=np.packbits(kept.cpu().numpy()),
        densities=_stored(densities.reshape(-1)[labels != LABEL_PRUNED], store_dtype, "the densities of the voxels that stay"),
        kept_features=_stored(features.reshape(-1, F)[kept], store_dtype, "the features of the kept voxels").reshape(-1, F),
        indices=index.cpu().numpy().astype(np.uint16), codebook=codebook.cpu().numpy().astype(np.float32).reshape(-1, F),
        empty_density=float(empty_density),
        dtypes=(str(densities.dtype).replace("torch.", ""), str(features.dtype).replace("torch.", "")),
        distortion=tuple(float(v) for v in distortion))


def decompress(compressed: CompressedGrid) -> Tuple[Tensor, Tensor]:
    """(densities [X,Y,Z,1], features [X,Y,Z,F]) float32 on the CPU: pruned voxels get the empty density and zero features, VQ
    voxels codebook[index], kept voxels and all densities that stay the stored values widened to float32"""
    labels = torch.from_numpy(compressed.labels().reshape(-1))
    n, F = labels.numel(), int(compressed.feature_dims)
    dens = torch.full((n,), float(compressed.empty_density), dtype=torch.float32)
    dens[labels != LABEL_PRUNED] = torch.from_numpy(compressed.densities.astype(np.float32))
    feat = torch.zeros((n, F), dtype=torch.float32)
    feat[labels == LABEL_KEPT] = torch.from_numpy(compressed.kept_features.astype(np.float32)).reshape(-1, F)
    codebook = torch.from_numpy(compressed.codebook.astype(np.float32)).reshape(-1, F)
    feat[labels == LABEL_VQ] = codebook[torch.from_numpy(compressed.indices.astype(np.int64))]
    return dens.reshape(*compressed.dims, 1), feat.reshape(*compressed.dims, F)


# ---- the file -------------------------------------------------------------------------------------------------------------------
def _deflate(arr: np.ndarray) -> Dict[str, Any]:
    arr = np.ascontiguousarray(arr)
    return {"data": zlib.compress(arr.tobytes(), 9), "dtype": str(arr.dtype), "shape": tuple(int(v) for v in arr.shape)}


def _inflate(entry: Dict[str, Any]) -> np.ndarray:
    return np.frombuffer(zlib.decompress(entry["data"]), dtype=np.dtype(entry["dtype"])).reshape(entry["shape"]).copy()


def to_entry(compressed: CompressedGrid) -> Dict[str, Any]:
    """the `compressed` checkpoint entry: plain python values and deflated arrays (bytes, dtype, shape)"""
    entry = {f.name: getattr(compressed, f.name) for f in dataclasses.fields(compressed) if f.name not in compressed.ARRAYS}
    entry.update({name: _deflate(getattr(compressed, name)) for name in compressed.ARRAYS})
    return entry


def from_entry(entry: Dict[str, Any]) -> CompressedGrid:
    values = {k: (_inflate(v) if k in CompressedGrid.ARRAYS else v) for k, v in entry.items()}
    values["dims"] = tuple(int(v) for v in values["dims"])
    return CompressedGrid(**values)


def is_compressed(model_data: Dict[str, Any]) -> bool:
    return COMPRESSED in model_data.get(THRE3D_REPR, {})


def compress_checkpoint_(model_data: Dict[str, Any], compressed: CompressedGrid) -> Dict[str, Any]:
    """Replace, in place, the density and feature tensors of a loaded checkpoint dict by the `compressed` entry; every other
    entry (render config, extra info, background, exposure, the grid's config) is left as it is"""
    state = model_data[THRE3D_REPR][STATE_DICT]
    if u_ATTN in state:
        raise ValueError("checkpoints that carry attention parameters (a keep grid) cannot be compressed")
    for key in (u_DENSITIES, u_FEATURES):
        del state[key]
    model_data[THRE3D_REPR][COMPRESSED] = to_entry(compressed)
    return model_data


def expand_checkpoint_(model_data: Dict[str, Any]) -> bool:
    """Turn, in place, a checkpoint dict with a `compressed` entry back into an ordinary one (the state dict gets its density
    and feature tensors in the dtypes they had, the entry goes); False, and nothing is touched, for a dict without the entry"""
    if not is_compressed(model_data):
        return False
    compressed = from_entry(model_data[THRE3D_REPR].pop(COMPRESSED))
    dens, feat = decompress(compressed)
    state = model_data[THRE3D_REPR][STATE_DICT]
    state[u_DENSITIES] = dens.to(getattr(torch, compressed.dtypes[0]))
    state[u_FEATURES] = feat.to(getattr(torch, compressed.dtypes[1]))
    return True


def save_compressed(path, model_data: Dict[str, Any], compressed: CompressedGrid) -> None:
    """Write the checkpoint dict `model_data` (as torch.load returned it) with its grid tensors replaced by `compressed`"""
    torch.save(compress_checkpoint_(model_data, compressed), path)


def load_compressed(path) -> Tuple[Dict[str, Any], CompressedGrid]:
    """(checkpoint dict, CompressedGrid) of a file written by save_compressed; the dict keeps its `compressed` entry"""
    model_data = torch.load(path, map_location="cpu", weights_only=False)
    if not is_compressed(model_data):
        raise ValueError(f"{path} holds no compressed voxel grid")
    return model_data, from_entry(model_data[THRE3D_REPR][COMPRESSED])


def load_uncompressed_checkpoint(path) -> Dict[str, Any]:
    """torch.load for the tools that rewrite a checkpoint's grid tensors in place: ValueError that names the decompression
    tool for a compressed file"""
    model_data = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(model_data, dict) and is_compressed(model_data):
        raise ValueError(f"{path} is a compressed checkpoint: this tool rewrites the grid tensors of the file and needs them "
                         f"in full.  Run {DECOMPRESS_TOOL} -i {path} -o <model.pth> first and pass its output.")
    return model_data


def checkpoint_bytes(model_data: Dict[str, Any]) -> int:
    """size of the file torch.save writes for the dict"""
    import io

    buffer = io.BytesIO()
    torch.save(model_data, buffer)
    return buffer.getbuffer().nbytes
