"""The random affine + thin-plate-spline transform of the equivariance term (Transform,
trainer.py:91-129 of Luh1124/face-vae; from FOMM) over ops_tps.

The constructor makes the reference's two torch.normal draws in its order from the default CPU
generator, so after torch.manual_seed(s) it holds the reference's theta and control_params bit for
bit.  theta [bs, 2, 3], control_params [bs, 1, points_tps^2] and control_points
[1, points_tps, points_tps, 2] are plain fp32 tensors read at call time (callers may overwrite
them); each call copies theta and control_params to the device of its argument.  The kernels
compute the control lattice themselves: control_points is kept for callers that read it.
"""
from __future__ import annotations

import torch

from . import ops_tps
from .warp import make_coordinate_grid_2d


class Transform:
    def __init__(self, bs, sigma_affine=0.05, sigma_tps=0.005, points_tps=5):
        noise = torch.normal(mean=0, std=sigma_affine * torch.ones([bs, 2, 3]))
        self.theta = noise + torch.eye(2, 3).view(1, 2, 3)
        self.bs = bs
        self.control_points = make_coordinate_grid_2d((points_tps, points_tps)).unsqueeze(0)
        self.control_params = torch.normal(mean=0, std=sigma_tps * torch.ones([bs, 1, points_tps ** 2]))

    def _on(self, device):
        """theta, control_params on `device` and the lattice size they imply."""
        pts = self.control_points.shape[1]
        if self.control_params.shape[-1] != pts * pts:
            raise ValueError(f"facevae_amd Transform: control_params {tuple(self.control_params.shape)} does not match "
                             f"the {pts} x {pts} control lattice")
        return self.theta.to(device), self.control_params.to(device), pts

    def transform_frame(self, frame):
        """frame [bs, C, H, W] (any float dtype) -> F.grid_sample(frame, warp_coordinates(grid),
        align_corners=True, padding_mode="reflection"), NCHW fp32.  The frame is data: no gradient."""
        if frame.requires_grad:
            raise ValueError("facevae_amd Transform.transform_frame: the frame is data (trainer.py:271-272); "
                             "a frame that requires grad is not supported")
        if frame.dim() != 4 or frame.shape[0] != self.bs:
            raise ValueError(f"facevae_amd Transform.transform_frame: a frame [{self.bs}, C, H, W] is expected, "
                             f"got {tuple(frame.shape)}")
        theta, cparams, pts = self._on(frame.device)
        return ops_tps.warp_frame(frame, theta, cparams, pts)

    def warp_coordinates(self, coordinates):
        """coordinates [bs, M, 2] or [1, M, 2] -> [bs, M, 2]; differentiable in the coordinates."""
        if coordinates.dim() != 3 or coordinates.shape[2] != 2 or coordinates.shape[0] not in (1, self.bs):
            raise ValueError(f"facevae_amd Transform.warp_coordinates: coordinates [{self.bs}, M, 2] or [1, M, 2] "
                             f"are expected, got {tuple(coordinates.shape)}")
        theta, cparams, pts = self._on(coordinates.device)
        # the broadcast form is expanded here, in front of the Function, so autograd sums its gradient
        coordinates = coordinates.expand(self.bs, -1, -1)
        return ops_tps.WarpCoordsFn.apply(coordinates, theta, cparams, pts)
