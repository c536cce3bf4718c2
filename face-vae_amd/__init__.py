"""facevae_amd — MI355X-native (gfx950) FaceVAE training step.

Import as `facevae_amd` (see `load_package()` in the repo root's __graft_entry__.py, or
`import fvamd` which registers the package under that name).

Hot path: AFE 2-D trunk -> latent split/reparam -> Generator 2-D trunk,
MSE + KL, Adam; every compute op is a hand-written HIP kernel in libfacevae.so called
through the C-ABI in include/facevae.h.
"""
from . import _lib
from .config import FaceVAEConfig, compute_dtype, set_compute_dtype
from .losses import (ContrastiveLoss_linear, DeformationPriorLoss, EquivarianceLoss, FeatureMatchingLoss, GANLoss, HeadPoseLoss,
                     KeypointPriorLoss, KLDivergenceLoss, L1Loss, PerceptualLoss, ReconLoss)
from .models import AFE, CKD, EFE_conv5, HPE_EDE, MFE, Discriminator, FaceVAE, Generator
from .modules import (Conv2d, Conv3d, ConvBlock2D, ConvBlock3D, ConvTranspose2dELR, DownBlock2D, DownBlock3D,
                      MaxPool2d, ResBlock2D, ResBlock3D, ResBottleneck, SameBlock2D, SameBlock3D, UpBlock2D, UpBlock3D)
from .optim import Adam
from .pose import rotation_matrix_x, rotation_matrix_y, rotation_matrix_z, transform_kp, transform_kp_with_new_pose
from . import animate, checkpoint, distributed, graph, ops, ops3d, ops_ckd, ops_efe, ops_hopenet, ops_pose, ops_tps, pose, warp
from .transform import Transform
from .hopenet import Hopenet
from .animate import Animator, CapturedDrive
from .graph import StepGraph

__all__ = ["FaceVAEConfig", "compute_dtype", "set_compute_dtype", "KLDivergenceLoss", "L1Loss", "PerceptualLoss", "ReconLoss",
           "AFE", "FaceVAE", "Generator", "Conv2d", "ConvBlock2D", "ConvTranspose2dELR", "DownBlock2D", "ResBlock2D", "ResBlock3D", "ConvBlock3D", "SameBlock2D",
           "UpBlock2D", "Adam", "distributed", "ops", "FaceVAETrainer", "Discriminator", "GANLoss", "FeatureMatchingLoss",
           "MFE", "DownBlock3D", "UpBlock3D", "Conv3d", "HPE_EDE", "ResBottleneck", "MaxPool2d", "HeadPoseLoss",
           "transform_kp", "rotation_matrix_x", "rotation_matrix_y", "rotation_matrix_z", "ops_pose", "pose",
           "CKD", "EquivarianceLoss", "KeypointPriorLoss", "DeformationPriorLoss", "ops_ckd",
           "EFE_conv5", "SameBlock3D", "ContrastiveLoss_linear", "ops_efe",
           "Transform", "ops_tps", "Hopenet", "ops_hopenet",
           "Animator", "CapturedDrive", "animate", "transform_kp_with_new_pose"]


def __getattr__(name):
    if name == "FaceVAETrainer":
        from .trainer import FaceVAETrainer
        return FaceVAETrainer
    raise AttributeError(name)
