"""Surface normals from the analytic gradient of the density field.

    sigma, grad = density_gradient(system, points)            # [M], [M, 3]: sigma_s and d sigma_s / d x at world points
    normal = normal_composite(grad, w_s)                       # [R, 3]: per-ray normal from per-sample gradients and weights
    res = render_rays(..., normals=True)["normal_fine"]        # the same, at the pass's own samples
    mesh = geometry.refine_normals(system, mesh)               # vertex normals from the field instead of the grid

The field is an MLP of a BARF-masked sinusoidal encoding, so its gradient exists in closed form.  `upnerf_density_grad`
(csrc/normals.hip) evaluates density and gradient in one fused launch: the tile's activations stay in LDS, the ReLU decisions
in registers, and the walk back through the transposed weights happens in the same kernel -- nothing of size M x W touches
HBM.  It runs the fp32 MFMA whatever the field mode of the training step.  The kernel reads the parameters in fragment order
and as transposed fragments, so a call re-packs them first (three launches over the parameter vector); inside a
`reuse_fragments()` block, which render_path opens round its chunks, that happens once per field and every later call is the
one launch.

Conventions: gradients and normals are in WORLD space; a normal is -grad / |grad| (it points towards lower density, out of the
surface, as the mesh normals do); where the gradient is zero or not finite the normal is (0, 0, 0), which the normal map draws
as mid-grey.  Everything here runs on the GPU only."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .ops import TIMER
from .static_scene import field_of, require_cuda

__all__ = ["density_gradient", "field_density_gradient", "normal_composite", "sample_points", "reuse_fragments", "TILE"]

TILE = 64  # points per workgroup of upnerf_density_grad (NORMALS_TILE)


_REUSE: Optional[dict] = None  # id(model) -> (P fragments, transposed fragments) while a reuse_fragments() block is open


@contextlib.contextmanager
def reuse_fragments():
    """While the block is open every field is re-packed for upnerf_density_grad once instead of once per call (three launches
    over its parameter vector each time).  For loops that do not change parameters between calls -- the chunks of
    render_path.  Not automatic: the optimiser kernels write parameters through raw pointers, so no version counter could
    tell a stale copy from a fresh one."""
    global _REUSE
    outer, _REUSE = _REUSE, ({} if _REUSE is None else _REUSE)
    try:
        yield
    finally:
        _REUSE = outer


def _fragments(model) -> Tuple[torch.Tensor, torch.Tensor]:
    """(P in fragment order, transposed fragments) of `model`: packed here, or taken from the open reuse_fragments() block."""
    if _REUSE is not None and id(model) in _REUSE:
        return _REUSE[id(model)][1:]
    pk = model.packer
    P = model.packed().detach().contiguous()
    out = (pk.frag_hip(P), pk.frag_t_hip(P))
    if _REUSE is not None:
        _REUSE[id(model)] = (model,) + out  # (the module is held so that its id stays its own)
    return out


@torch.no_grad()
def field_density_gradient(model, points: torch.Tensor, wk_xyz=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma [M], grad [M, 3]) of one NeRF module at `points` [M, 3] (fp32 device tensor): upnerf_density_grad with the
    module's packed parameters.  wk_xyz: the ten band weights; default: those of the module's progress."""
    from .rendering import band_weights
    require_cuda("density_gradient", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points is a fp32 tensor [M, 3]")
    points = points.detach().contiguous()
    M, dev = points.shape[0], points.device
    sigma = torch.empty(M, device=dev, dtype=torch.float32)
    grad = torch.empty(M, 3, device=dev, dtype=torch.float32)
    if M == 0:
        return sigma, grad
    pk = model.packer
    if wk_xyz is None:
        wk_xyz = band_weights(model.xyz_L, model.host_progress_value(), model.c2f)
    PF, PT = _fragments(model)
    a = _lib.DensityGradArgs(M=M, points=ptr(points), P=ptr(PF), PT=ptr(PT), wk_xyz=(C.c_float * 10)(*wk_xyz), sigma=ptr(sigma),
                             grad=ptr(grad))
    st = stream()
    check(TIMER.run("density_grad", lambda: lib.upnerf_density_grad(C.byref(pk.L), C.byref(a), st), units=M), "upnerf_density_grad")
    return sigma, grad


def density_gradient(system, points: torch.Tensor, field: str = "fine") -> Tuple[torch.Tensor, torch.Tensor]:
    """(sigma [M], grad [M, 3]): the shared density (sigma_s, after the softplus) of the `field` ("fine" or "coarse") network
    at the world points `points` [M, 3] and its gradient d sigma / d x there, with the BARF band weights of the model's
    current progress (as geometry.density_grid takes them).  GPU only; raises what density_grid raises."""
    model, dev = field_of(system, field, "density_gradient")
    points = torch.as_tensor(points)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points is a tensor [M, 3]")
    return field_density_gradient(model, points.to(device=dev, dtype=torch.float32))


@torch.no_grad()
def normal_composite(grad: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[R, 3]: normalise(sum_i w[r, i] * (-grad[r, i] / |grad[r, i]|)) (upnerf_normal_composite).  grad [R * S, 3] or [R, S, 3],
    w [R, S]: fp32 device tensors.  Terms with a zero or non-finite gradient count as zero; a zero sum gives (0, 0, 0)."""
    require_cuda("normal_composite", grad, w)
    if w.dim() != 2 or grad.numel() != 3 * w.numel() or grad.shape[-1] != 3:
        raise ValueError(f"expected grad [R * S, 3] and w [R, S]; got {tuple(grad.shape)} and {tuple(w.shape)}")
    R, S = w.shape
    grad, w = grad.detach().contiguous().float(), w.detach().contiguous().float()
    out = torch.empty(R, 3, device=w.device, dtype=torch.float32)
    if R == 0:
        return out
    a = _lib.NormalCompositeArgs(R=R, S=S, grad=ptr(grad), w=ptr(w), normal=ptr(out))
    st = stream()
    check(TIMER.run("normal_composite", lambda: lib.upnerf_normal_composite(C.byref(a), st), units=R * S), "upnerf_normal_composite")
    return out


def sample_points(rays_o: torch.Tensor, rays_d: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """[R * S, 3]: o + d z with the two roundings the field kernels give it (a product, then a sum)."""
    return (rays_o.detach()[:, None, :] + rays_d.detach()[:, None, :] * z.detach()[:, :, None]).reshape(-1, 3)
