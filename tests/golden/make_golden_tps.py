"""Generate the golden fixture of the equivariance transform FROM THE REFERENCE ITSELF.

Run where the reference checkout is available (see make_golden.py), on the CPU:

    python tests/golden/make_golden_tps.py

Imports the reference `trainer.py` / `utils.py` / `losses.py` read-only (the inert torchvision
placeholder of make_golden.import_reference is enough: trainer.py touches torchvision only inside
GeneratorFull.__init__).  `make_coordinate_grid_2d` calls `.cuda()` (utils.py:81-82); for the
duration of this script torch.Tensor.cuda is the identity (the arithmetic is unchanged: CPU fp32).
Stores plain tensors in tests/golden/tps.pt (loaded with weights_only=True):

  ctor      Transform(bs) after torch.manual_seed(seed): theta, control_params, control_points for
            (seed 7, bs 2) and (seed 11, bs 3, points_tps 3)
  frame     cases a-e (table in FRAMES): the seeded torch.rand frame, theta, control_params, the
            reference's transform_frame output, and two scalars computed here: `ref_dev`, the rel-L2
            deviation of the reference's fp32 output from the fp64 restatement of the same formulas
            (tests/tps_reference.py), and `outside`, the share of output pixels whose warped
            coordinate leaves [-1, 1].  Asserted: outside >= 0.05 for a, >= 0.5 for b and c
  coords    warp_coordinates and its gradient (torch autograd, loss sum(out * g)) on seeded points
            [2, 5, 2] and [3, 15, 2] in [-1, 1] and on a set placed on the lattice: points equal to a
            control point, points sharing exactly one coordinate with one, a point outside [-1, 1];
            `ref_dev` of both results
  chain     EquivarianceLoss()(kp_d, transform.warp_coordinates(transformed_kp[:, :, :2])) on [3, 5, 3]
            keypoints, with both input gradients
  workload  [2, 3, 256, 256], default sigmas: the seeds, theta, control_params and ref_dev only (the
            test regenerates the frame from its seed)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402  (puts tests/ on sys.path)
import tps_reference as R  # noqa: E402

SEED = 7
# case: frame shape, frame seed, sigma_affine, sigma_tps, points_tps, least share of pixels outside [-1, 1]
FRAMES = {
    "a": ((2, 3, 20, 28), 701, 0.05, 0.005, 5, 0.05),   # the reference's own setting; H != W
    "b": ((2, 3, 20, 28), 702, 0.8, 0.05, 5, 0.5),      # about half the pixels reflect
    "c": ((3, 5, 37, 53), 703, 1.5, 0.1, 5, 0.5),       # coordinates to about +-9: several flips; odd sizes
    "d": ((1, 1, 5, 9), 704, 0.05, 0.005, 5, 0.0),      # columns 0, 2, 4, 6, 8 sit on control points
    "e": ((2, 3, 16, 24), 705, 0.05, 0.005, 3, 0.0),    # points_tps = 3
}
WORKLOAD = ((2, 3, 256, 256), 706)


def pts_of(t):
    return t.control_points.shape[1]


def coords_case(trainer, seed, bs, coords, g, sig=(0.05, 0.005), pts=5):
    torch.manual_seed(seed)
    t = trainer.Transform(bs, *sig, points_tps=pts)
    c = coords.clone().requires_grad_(True)
    out = t.warp_coordinates(c)
    (out * g).sum().backward()
    o64, d64 = R.coords_with_grad(coords, g, t.theta, t.control_params, pts)
    dev = dict(out=torch.tensor(R.rel_l2(out, o64)), d_coords=torch.tensor(R.rel_l2(c.grad, d64)))
    return dict(coords=coords, g=g, theta=t.theta, control_params=t.control_params, points_tps=torch.tensor(pts),
                out=out.detach(), d_coords=c.grad.clone(), ref_dev=dev)


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # make_coordinate_grid_2d calls .cuda()
    _, _, losses = import_reference()
    import trainer  # noqa: E402  (reference)
    torch.set_num_threads(8)
    out = {}

    ctor = {}
    for name, seed, bs, kw in (("s7", 7, 2, {}), ("s11", 11, 3, dict(points_tps=3))):
        torch.manual_seed(seed)
        t = trainer.Transform(bs, **kw)
        ctor[name] = dict(seed=torch.tensor(seed), bs=torch.tensor(bs), points_tps=torch.tensor(pts_of(t)),
                          theta=t.theta, control_params=t.control_params, control_points=t.control_points)
    out["ctor"] = ctor

    frames = {}
    for name, (shape, fseed, sa, st, pts, least) in FRAMES.items():
        torch.manual_seed(SEED)
        t = trainer.Transform(shape[0], sa, st, points_tps=pts)
        x = torch.rand(shape, generator=torch.Generator().manual_seed(fseed))
        y = t.transform_frame(x)
        dev = R.rel_l2(y, R.transform_frame(x, t.theta, t.control_params, pts))
        outside = R.outside_share(shape[2], shape[3], t.theta, t.control_params, pts)
        print(f"frame {name} {list(shape)}: outside {outside:.3f}  ref_dev {dev:.2e}")
        assert outside >= least, (name, outside, least)
        frames[name] = dict(x=x, theta=t.theta, control_params=t.control_params, points_tps=torch.tensor(pts), y=y,
                            ref_dev=torch.tensor(dev), outside=torch.tensor(outside))
    out["frame"] = frames

    gen = torch.Generator().manual_seed(711)
    rnd = lambda *s: (torch.rand(*s, generator=gen) - 0.5) * 2          # noqa: E731
    cs = {}
    cs["a"] = coords_case(trainer, SEED, 2, rnd(2, 5, 2), torch.randn(2, 5, 2, generator=gen))
    cs["b"] = coords_case(trainer, SEED, 3, rnd(3, 15, 2), torch.randn(3, 15, 2, generator=gen), sig=(0.3, 0.05))
    lattice = torch.tensor([[0.0, 0.0], [-1.0, 1.0], [0.5, -0.5],        # control points
                            [0.5, 0.3], [0.13, -1.0], [-0.7, 0.0],       # one coordinate shared
                            [1.7, -0.2]])                                # outside [-1, 1]
    cs["lattice"] = coords_case(trainer, SEED, 2, lattice.unsqueeze(0).repeat(2, 1, 1),
                                torch.randn(2, lattice.shape[0], 2, generator=gen), sig=(0.3, 0.05))
    for k, v in cs.items():
        print(f"coords {k} {list(v['coords'].shape)}: ref_dev out {v['ref_dev']['out']:.2e}  "
              f"d_coords {v['ref_dev']['d_coords']:.2e}")
    out["coords"] = cs

    gen = torch.Generator().manual_seed(712)
    kp_d = rnd(3, 5, 3)
    tkp = rnd(3, 5, 3)
    torch.manual_seed(SEED)
    t = trainer.Transform(3, 0.3, 0.05)
    a, b = kp_d.clone().requires_grad_(True), tkp.clone().requires_grad_(True)
    loss = losses.EquivarianceLoss()(a, t.warp_coordinates(b[:, :, :2]))
    loss.backward()
    out["chain"] = dict(kp_d=kp_d, transformed_kp=tkp, theta=t.theta, control_params=t.control_params,
                        loss=loss.detach(), d_kp_d=a.grad.clone(), d_transformed_kp=b.grad.clone())

    shape, fseed = WORKLOAD
    torch.manual_seed(SEED)
    t = trainer.Transform(shape[0])
    x = torch.rand(shape, generator=torch.Generator().manual_seed(fseed))
    dev = R.rel_l2(t.transform_frame(x), R.transform_frame(x, t.theta, t.control_params, 5))
    print(f"workload {list(shape)}: ref_dev {dev:.2e}")
    out["workload"] = dict(shape=torch.tensor(shape), frame_seed=torch.tensor(fseed), seed=torch.tensor(SEED),
                           theta=t.theta, control_params=t.control_params, ref_dev=torch.tensor(dev))

    for path in save_golden(out, "tps.pt"):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
