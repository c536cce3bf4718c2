"""Restatement of the reference's Transform (trainer.py:91-129 of Luh1124/face-vae) in torch CPU
ops, at a chosen precision: what tests/test_tps_gpu.py compares the kernels against in fp64, and
what tests/test_tps_cpu.py pins against the reference's own fp32 results (tests/golden/tps.pt).

Every function takes theta [B, 2, 3] and control_params [B, 1, P*P] (or [B, P*P]) and works in
`dtype`; nothing here calls the product's kernels.
"""
import torch
import torch.nn.functional as F

F64 = torch.float64


def grid_2d(h, w, dtype=F64):
    """make_coordinate_grid_2d (utils.py:79-88): [h, w, 2] of (x over w, y over h) in [-1, 1].  The
    reference divides in fp32 (an int64 arange over a Python int); `dtype` divides in `dtype`."""
    x = 2 * (torch.arange(h).to(dtype) / (h - 1)) - 1
    y = 2 * (torch.arange(w).to(dtype) / (w - 1)) - 1
    return torch.stack([y.view(1, -1).expand(h, w), x.view(-1, 1).expand(h, w)], dim=2)


def warp_coordinates(coords, theta, control_params, pts, dtype=F64):
    """trainer.py:112-129.  coords [B, M, 2] or [1, M, 2] -> [B, M, 2]."""
    B = theta.shape[0]
    coords, theta = coords.to(dtype), theta.to(dtype).unsqueeze(1)
    cparams = control_params.to(dtype).reshape(B, 1, pts * pts)
    cpoints = grid_2d(pts, pts, dtype).reshape(1, 1, pts * pts, 2)
    out = (torch.matmul(theta[:, :, :, :2], coords.unsqueeze(-1)) + theta[:, :, :, 2:]).squeeze(-1)   # :115-116
    d = (coords.reshape(coords.shape[0], -1, 1, 2) - cpoints).abs().sum(-1)                          # :120-121
    r = d ** 2 * torch.log(d + 1e-6) * cparams                                                       # :123-125
    return out + r.sum(dim=2).reshape(B, coords.shape[1], 1)                                         # :126-127


def warped_grid(h, w, theta, control_params, pts, dtype=F64):
    """The sampling grid of transform_frame (trainer.py:107-109): [B, h, w, 2]."""
    g = grid_2d(h, w, dtype).reshape(1, h * w, 2)
    return warp_coordinates(g, theta, control_params, pts, dtype).reshape(theta.shape[0], h, w, 2)


def transform_frame(frame, theta, control_params, pts, dtype=F64):
    """trainer.py:106-110."""
    grid = warped_grid(frame.shape[2], frame.shape[3], theta, control_params, pts, dtype)
    return F.grid_sample(frame.to(dtype), grid, align_corners=True, padding_mode="reflection")        # :110


def outside_share(h, w, theta, control_params, pts):
    """Share of output pixels whose warped coordinate leaves [-1, 1] (the reflection branch)."""
    g = warped_grid(h, w, theta, control_params, pts)
    return (g.abs() > 1).any(dim=3).double().mean().item()


def coords_with_grad(coords, g_out, theta, control_params, pts, dtype=F64):
    """-> (out, d_coords) for the loss sum(out * g_out), by torch autograd."""
    c = coords.detach().to(dtype).requires_grad_(True)
    out = warp_coordinates(c, theta, control_params, pts, dtype)
    (out * g_out.to(dtype)).sum().backward()
    return out.detach(), c.grad


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
