"""Reenact a driving clip with a source face from a reference checkpoint: the job of the
reference's evaluate.py, with its flags, on facevae_amd.Animator.

    python tools/animate.py --ckp_dir ckp --ckp 100 --source r --driving clip/ --output out.gif

--source r   reconstruction: the first driving frame is the source, the others drive it
--source f   frontalisation: every frame is its own source, re-posed to (yaw, pitch, roll) = 0
--source P   the image file P, resized to 256 x 256 (nearest, as evaluate.py), driven by every frame
--driving    a folder of frames (sorted by name) or a .gif; the first --num_frames are used
--output     a .gif (written through PIL), or a .npy of the [T, H, 2W, 3] uint8 frames

--graph      capture the per-frame call once (Animator.capture, uint8 in and out) and stream the clip through
             its replays, --batch frames per replay, uploads and downloads overlapping them; the last,
             shorter chunk runs eagerly.  Not with --source f, which changes the source every frame.

Each output frame is the driving frame on the left and the generated one on the right.  The
checkpoint is <ckp_dir>/<ckp zero-filled to 8>-checkpoint.pth.tar as Logger.save_cpk writes it; its
afe / ckd / hpe_ede / mfe / generator entries are loaded strictly (--efe: the efe entry too, whose
keypoint refinement GeneratorFull.forward applies).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fvamd  # noqa: E402,F401
import facevae_amd as fv  # noqa: E402
from facevae_amd import checkpoint, data  # noqa: E402


def to_nchw(frames_u8):
    """[T, H, W, 3] uint8 (numpy) -> [T, 3, H, W] fp32 in [0, 1] on the GPU (img_as_float32's scaling)."""
    t = torch.from_numpy(np.array(frames_u8)).cuda()      # a copy: PIL hands out read-only arrays
    return t.permute(0, 3, 1, 2).float().mul_(float(data.INV255)).contiguous()


def write_frames(path, frames):
    if path.lower().endswith(".npy"):
        np.save(path, frames)
        return
    from PIL import Image
    ims = [Image.fromarray(f) for f in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], loop=0, duration=40)


def main():
    ap = argparse.ArgumentParser(description="face-vid2vid reenactment (facevae_amd.Animator)")
    ap.add_argument("--ckp_dir", type=str, default="ckp", help="Checkpoint dir")
    ap.add_argument("--output", type=str, default="output.gif", help="Output .gif or .npy")
    ap.add_argument("--ckp", type=int, default=0, help="Checkpoint epoch")
    ap.add_argument("--source", type=str, default="r",
                    help="Source image, f for face frontalization, r for reconstruction")
    ap.add_argument("--driving", type=str, required=True, help="Driving dir or .gif")
    ap.add_argument("--num_frames", type=int, default=90, help="Number of frames")
    ap.add_argument("--batch", type=int, default=8, help="driving frames per call")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--efe", action="store_true", help="load and apply the checkpoint's efe entry")
    ap.add_argument("--graph", action="store_true", help="replay a captured HIP graph per chunk of --batch frames")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("animate needs a GPU")
    if a.graph and a.source == "f":
        raise SystemExit("--graph drives one source with every frame; --source f takes a new source per frame")
    models = checkpoint.load_reference_models(checkpoint.reference_checkpoint_path(a.ckp_dir, a.ckp), efe=a.efe)
    mode = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    for m in models.values():
        m.cuda().eval().set_compute_dtype(mode)
    anim = fv.Animator(models["afe"], models["ckd"], models["hpe_ede"], models["mfe"], models["generator"],
                       models.get("efe"))
    video = data.read_video_u8(a.driving)[:a.num_frames]
    out = []
    if a.source == "f":
        for i in range(len(video)):
            frame = to_nchw(video[i:i + 1])
            out.append(anim.set_source(frame).drive(frame, new_pose=(0.0, 0.0, 0.0), as_uint8=True).cpu().numpy())
    else:
        if a.source == "r":
            source, video = to_nchw(video[:1]), video[1:]
        else:
            source = to_nchw(data._read_frame_u8(a.source)[None])
            source = torch.nn.functional.interpolate(source, size=(256, 256))
        anim.set_source(source)
        whole = len(video) // a.batch * a.batch if a.graph else 0
        if whole:
            cap = anim.capture(a.batch, as_uint8=True, u8_in=True)
            out.extend(cap.stream(np.array(video[i:i + a.batch]) for i in range(0, whole, a.batch)))
        for i in range(whole, len(video), a.batch):
            out.append(anim.drive(to_nchw(video[i:i + a.batch]), as_uint8=True, fused_pose=a.graph).cpu().numpy())
    if not out:
        raise SystemExit(f"{a.driving}: no driving frames")
    write_frames(a.output, np.concatenate(out))
    print(f"wrote {a.output}: {sum(len(o) for o in out)} frames")


if __name__ == "__main__":
    main()
