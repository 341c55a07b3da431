"""The ways a grid can change between two calls through one workspace (torch only, any device), shared by
tests/test_cache_keys_host.py (CPU: what `Workspace.holds` decides) and tests/test_cache_coherence_gpu.py (GPU: what the kernels
then read).

A change takes an `Owner` -- the two grid tensors as a caller holds them, with VoxelGrid's surface (`densities` / `features`
properties with setters, `spec`) and none of its cache invalidation, so that a row checks the workspace's own decision -- and
mutates or replaces what it owns.  The same functions run on a `VoxelGrid` where `Change.on_grid` says so.  Every change moves the
values far enough to show in a render (max |delta colour| > 1e-2 on the GPU module's scene).

Rows that depend on the allocator handing a freed block back (`reuses_address`) ASSERT that they produced the hazard: the new tensor
has the old one's `data_ptr` and `_version`.  `alloc_at` keeps its misses alive until a request lands on the wanted block."""
import dataclasses
import weakref
from typing import Callable

import numpy as np
import torch

from voxe_hip import abi, ops
from voxe_hip.runtime import f32c

DIMS = (20, 24, 28)
AABB = ((-1.5, 1.5),) * 3
SCALE = 3.0
KINDS = {"sh0": (3, abi.FEAT_SH, 0), "sh1": (12, abi.FEAT_SH, 1), "attn": (1, abi.FEAT_ATTN, 0)}   # F, feature_kind, sh_degree
SOURCES = ("f32", "f64", "f16", "permuted")


def base_spec(kind: str) -> ops.GridSpec:
    return ops.GridSpec(aabb=AABB, density_scale=SCALE, density_pre_act=abi.ACT_IDENTITY, density_post_act=abi.ACT_SOFTPLUS,
                        feature_kind=KINDS[kind][1])


def grid_values(kind: str):
    """(densities [X,Y,Z,1], features [X,Y,Z,F]) float32 numpy, U(-1, 1)"""
    F = KINDS[kind][0]
    rng = np.random.default_rng(61 + F)
    return (rng.uniform(-1, 1, DIMS + (1,)).astype(np.float32), rng.uniform(-1, 1, DIMS + (F,)).astype(np.float32))


def as_source(a: np.ndarray, source: str, device) -> torch.Tensor:
    """the values `a` as a tensor of the given kind: float32 contiguous, float64, float16 or a permuted (non-contiguous) view"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if source == "f64":
        return t.double().to(device)
    if source == "f16":
        return t.half().to(device)
    if source == "permuted":
        return t.permute(2, 1, 0, 3).contiguous().to(device).permute(2, 1, 0, 3)
    return t.to(device) if torch.device(device).type != "cpu" else host_tensor(a)


# On the device a freed block goes back to torch's caching allocator, which hands it to the next request of that size.  The host's
# malloc pads torch's aligned requests and does not take a lone hole of the exact size again, so the CPU tensors that rows replace
# live in blocks this module keeps and hands out again itself: {data_ptr: (the memory, weak reference to the storage over it)}.
_HOST_BLOCKS = {}


def host_tensor(a) -> torch.Tensor:
    """a CPU tensor with the values `a` (numpy array or tensor) in a block of this module's pool"""
    mem = np.array(a.detach().numpy() if isinstance(a, torch.Tensor) else a, copy=True, order="C")
    t = torch.from_numpy(mem)
    _HOST_BLOCKS[t.data_ptr()] = (mem, weakref.ref(t.untyped_storage()))
    return t


class Owner(torch.nn.Module):
    """the grid tensors as their owner sees them: VoxelGrid's tensor surface without its workspaces"""

    def __init__(self, densities: torch.Tensor, features: torch.Tensor, spec: ops.GridSpec, sh_degree: int = 0):
        super().__init__()
        self._densities = torch.nn.Parameter(densities)
        self._features = torch.nn.Parameter(features)
        self.spec = spec
        self.sh_degree = sh_degree
        self.guards = []

    @property
    def densities(self):
        return self._densities

    @densities.setter
    def densities(self, t):
        self._densities = t if isinstance(t, torch.nn.Parameter) else torch.nn.Parameter(t)

    @property
    def features(self):
        return self._features

    @features.setter
    def features(self, t):
        self._features = t if isinstance(t, torch.nn.Parameter) else torch.nn.Parameter(t)


def make_owner(kind: str, source: str = "f32", device="cpu") -> Owner:
    _HOST_BLOCKS.clear()           # (the owners before this one are gone)
    d, f = grid_values(kind)
    tensors = []
    guards = []
    fenced = torch.device(device).type == "cuda"
    for a in (d, f):
        # caching allocator: equal-sized neighbours on both sides, so that the block a dropped tensor leaves is not merged into a
        # larger free one (the host's malloc pads aligned requests: there a lone hole of the exact size is never taken again)
        if fenced:
            guards.append(as_source(a, source, device).clone())
        tensors.append(as_source(a, source, device))
        if fenced:
            guards.append(as_source(a, source, device).clone())
    owner = Owner(tensors[0], tensors[1], base_spec(kind), KINDS[kind][2])
    owner.guards = guards
    return owner


def make_voxel_grid(kind: str = "sh0", source: str = "f32", device="cpu"):
    """a tunable VoxelGrid over the same values (kind "sh0" | "sh1"), with the attention values of the "attn" kind"""
    from thre3d_atom.thre3d_reprs.voxels import VoxelGrid, VoxelSize

    o = make_owner(kind, source, device)
    grid = VoxelGrid(o.densities.detach(), o.features.detach(), VoxelSize(*(3.0 / n for n in DIMS)),
                     density_preactivation=torch.nn.Identity(), density_postactivation=torch.nn.Softplus(),
                     expected_density_scale=SCALE, tunable=True, attn=as_source(grid_values("attn")[1], "f32", device))
    grid.guards = o.guards
    grid.update_orig_densities()        # (until then the snapshot aliases the constructor's tensor and keeps its block in use)
    return grid


def alloc_at(ptr: int, make: Callable[[], torch.Tensor], tries: int = 256, misses=None) -> torch.Tensor:
    """a tensor from `make()` whose data_ptr is `ptr` (a block the allocator got back): misses stay alive until one lands there
    (in the caller's list `misses`, when given, for as long as the caller keeps it).
    Fails when none does: a test that cannot build the hazard tests nothing."""
    if ptr in _HOST_BLOCKS:
        mem, storage = _HOST_BLOCKS[ptr]
        values = make()
        assert storage() is None, "the block is still in use: its tensor was not dropped"
        assert values.numel() * values.element_size() == mem.nbytes
        block = mem.reshape(-1).view(values.numpy().dtype).reshape(tuple(values.shape))
        block[...] = values.numpy()
        t = torch.from_numpy(block)
        _HOST_BLOCKS[ptr] = (mem, weakref.ref(t.untyped_storage()))
        return t
    misses = [] if misses is None else misses
    for _ in range(tries):
        t = make()
        if t.data_ptr() == ptr:
            return t
        misses.append(t)
    raise AssertionError(f"no tensor of {tries} landed on the freed block at {ptr:#x}: the address-reuse hazard could not be built")


def converted_temporaries_collide(t: torch.Tensor, change: Callable[[], None], rounds: int = 16) -> bool:
    """the hazard of a converted input: does the dense float32 copy a call makes of `t` land on the address (and version) of the
    copy the call before made, although `change()` ran in between?  Up to `rounds` pairs of calls."""
    assert t.dtype != torch.float32 or not t.is_contiguous()
    seen = None
    for _ in range(rounds + 1):
        c = f32c(t.detach())
        now = (c.data_ptr(), c._version)
        del c
        if seen == now:
            return True
        seen = now
        change()
    return False


# ---- the changes ------------------------------------------------------------------------------------------------------------------
def _add(o):
    with torch.no_grad():
        o.densities.add_(0.5)


def _copy(o):
    with torch.no_grad():
        o.densities.copy_(o.densities.detach() + 0.5)


def _adam(o):
    # Adam's first step moves every element by lr against the sign of its gradient
    for p in (o.densities, o.features):
        p.grad = torch.ones_like(p)
    torch.optim.Adam([o.densities, o.features], lr=0.5).step()
    for p in (o.densities, o.features):
        p.grad = None


def _load_state_dict(o):
    state = {k: (v.detach() + 0.5 if k in ("_densities", "_features") else v.detach().clone()) for k, v in o.state_dict().items()}
    o.load_state_dict(state)


def _index_assign(o):
    with torch.no_grad():
        o.densities[:, :, 4:24] = o.densities.detach()[:, :, 4:24] + 1.0


def _setter_once(o):
    o.densities = o.densities.detach() + 0.5


def _setter_twice_same_address(o):
    ptr, version = o.densities.data_ptr(), o.densities._version
    o.densities = o.densities.detach() + 0.25          # (allocated while the old tensor lives: elsewhere; the old block is free now)
    first = o.densities.detach()
    o.densities = alloc_at(ptr, lambda: first + 0.25)
    assert (o.densities.data_ptr(), o.densities._version) == (ptr, version), "hazard not built"


def _del_then_fresh(o):
    """drop the features and build another tensor of the same size (bypassing the setters: nobody is told)"""
    ptr, version = o.features.data_ptr(), o.features._version
    values = o.features.detach().cpu() + 0.5
    device = o.features.device
    del o._features
    fresh = alloc_at(ptr, lambda: values.to(device, copy=True))
    assert (fresh.data_ptr(), fresh._version) == (ptr, version), "hazard not built"
    o._features = torch.nn.Parameter(fresh)


def _del_then_fresh_densities(o):
    ptr, version = o.densities.data_ptr(), o.densities._version
    values = o.densities.detach().cpu() + 0.5
    device = o.densities.device
    del o._densities
    fresh = alloc_at(ptr, lambda: values.to(device, copy=True))
    assert (fresh.data_ptr(), fresh._version) == (ptr, version), "hazard not built"
    o._densities = torch.nn.Parameter(fresh)


def _parameter_wrapping(o):
    """a fresh tensor wrapped by the caller; the plain handle and the Parameter share one version counter"""
    t = o.densities.detach() + 0.25
    p = torch.nn.Parameter(t)
    type(o).densities.fset(o, p)                        # (Module.__setattr__ would register a Parameter under the property's name)
    assert o.densities is p and p.data_ptr() == t.data_ptr() and p._version == t._version
    t.add_(0.25)                                        # written through the plain handle
    assert p._version == t._version


def _spec(**fields):
    def change(o):
        o.spec = dataclasses.replace(o.spec, **fields)
    return change


def _features_view_other_F(o):
    """SH-1 storage read as an SH-0 grid: same address, same version counter, another shape"""
    X, Y, Z, F = o.features.shape
    assert F == 12
    view = o.features.detach().reshape(-1)[: X * Y * Z * 3].view(X, Y, Z, 3)
    assert view.data_ptr() == o.features.data_ptr() and view._version == o.features._version
    o._features = torch.nn.Parameter(view)
    assert o._features.data_ptr() == view.data_ptr() and o._features._version == view._version
    o.sh_degree = 0


@dataclasses.dataclass(frozen=True)
class Change:
    name: str
    apply: Callable
    source: str = "f32"            # the kind of tensors the owner starts with (cache_cases.SOURCES)
    repack: bool = True            # the pack pass must run again (False: the change is outside the pack and must still show)
    reuses_address: bool = False   # the change itself asserts that a new tensor took an old one's (data_ptr, _version)
    on_grid: bool = True           # also meaningful on a VoxelGrid (same function, the grid's own setters)
    kinds: tuple = ("sh0", "sh1", "attn")
    gpu: bool = True               # False: no entry point renders both sides of the change (host decision only)


CHANGES = [
    # torch in-place writes
    Change("add_", _add),
    Change("copy_", _copy),
    Change("adam_step", _adam),
    Change("load_state_dict", _load_state_dict),
    Change("index_assignment", _index_assign),
    # replacement
    Change("setter_once", _setter_once),
    Change("setter_twice_same_address", _setter_twice_same_address, reuses_address=True),
    Change("del_then_fresh_features", _del_then_fresh, reuses_address=True),
    Change("del_then_fresh_densities", _del_then_fresh_densities, reuses_address=True),
    Change("parameter_wrapping", _parameter_wrapping),
    # converted inputs: the source changes in place between two calls
    Change("float64_source", _add, source="f64"),
    Change("float16_source", _add, source="f16"),
    Change("permuted_source", _add, source="permuted"),
    # spec changes on unchanged tensors
    Change("density_scale", _spec(density_scale=2.0 * SCALE), on_grid=False),
    Change("pre_activation", _spec(density_pre_act=abi.ACT_ABS), on_grid=False),
    Change("post_activation", _spec(density_post_act=abi.ACT_RELU), repack=False, on_grid=False),
    # (an attention grid needs F = 1 and an SH grid F = 3 (deg + 1)^2: no render accepts one tensor under both kinds)
    Change("feature_kind", _spec(feature_kind=abi.FEAT_ATTN), on_grid=False, kinds=("sh0",), gpu=False),
    Change("features_view_other_F", _features_view_other_F, on_grid=False, kinds=("sh1",)),
]
BY_NAME = {c.name: c for c in CHANGES}


def rows(gpu_only=False, grid_only=False):
    """[(change name, grid kind)] of the table"""
    return [(c.name, k) for c in CHANGES for k in c.kinds if (c.gpu or not gpu_only) and (c.on_grid or not grid_only)]


# ---- rays and jitter ----------------------------------------------------------------------------------------------------------------
def _rewrite(name):
    def change(r):
        r[name].add_(0.37 if name == "jitter" else 0.05)
        if name == "jitter":
            r[name].frac_()
    return change


def _replace_at_same_address(name):
    def change(r):
        old = r[name]
        ptr, version, device = old.data_ptr(), old._version, old.device
        values = old.cpu() + (0.37 if name == "jitter" else 0.05)
        if name == "jitter":
            values = values.frac()
        del old
        r[name] = None                                  # the caller drops its tensor ...
        r[name] = alloc_at(ptr, lambda: values.to(device, copy=True))      # ... and builds another one of the same size
        assert (r[name].data_ptr(), r[name]._version) == (ptr, version), "hazard not built"
    return change


RAY_CHANGES = {f"{how}_{name}": fn(name) for name in ("rays_o", "rays_d", "jitter")
               for how, fn in (("rewritten", _rewrite), ("replaced", _replace_at_same_address))}
