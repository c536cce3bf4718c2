"""Generate the golden fixture of the frozen Hopenet teacher FROM THE REFERENCE ITSELF.

Run where the reference checkout is available (see make_golden.py), on the CPU:

    python tests/golden/make_golden_hopenet.py

Imports the reference `trainer.py` read-only (the inert torchvision placeholder of
make_golden.import_reference is enough: Hopenet takes its block class as an argument, and this
script supplies tests/hopenet_reference.Bottleneck, torchvision's layout).  Hopenet.__init__ calls
`.cuda()` on idx_tensor (trainer.py:37); for the duration of this script torch.Tensor.cuda is the
identity (the arithmetic is unchanged: CPU fp32).

The weights are too large to commit (34 MB even for layers [1, 1, 1, 1]), so the fixture stores the
seeds of a recipe (tests/hopenet_reference.build / overwrite / make_inputs) and, per net of
hopenet_reference.NETS, in tests/golden/hopenet.pt (plain tensors, loaded with weights_only=True):

  state_sums   hopenet_reference.checksum of every state-dict entry after the recipe, in key order
  init_sums    the same straight after the seeded construction (the constructor's RNG draws)
  input_sum, prep_sum   checksums of the three 40 x 56 frames and of their 224 x 224 preprocessing
  angles [3, 3], features [3, 2048], taps (strided samples of the maps after the pool and after each
               layerL): the reference's outputs on the preprocessed frames
  max_prob     the largest softmax probability per head and image
  bf16_dev     (rel-L2 of the pooled features, max |angle difference| in rad) of
               hopenet_reference.emulate_bf16 against the fp32 outputs: the bf16 tests gate at 3 x these

and the state-dict keys with shapes in tests/golden/hopenet_keys.json.  Asserted here, so that the
tests are not blind: every largest probability lies in [0.05, 0.9]; the pooled features of any two
images differ by at least 0.05 rel-L2; any two images' angles differ by at least 1e-2 rad; the
restatement (hopenet_reference.RefHopenet, preprocess) reproduces the reference bit for bit.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, save_golden  # noqa: E402  (puts tests/ on sys.path)
import hopenet_reference as R  # noqa: E402


def main():
    torch.Tensor.cuda = lambda self, *a, **k: self       # Hopenet.__init__ calls .cuda()
    import_reference()
    import trainer  # noqa: E402  (reference)
    import utils  # noqa: E402  (reference)
    import torch.nn.functional as F
    torch.set_num_threads(8)

    frames = R.make_inputs()
    x = F.interpolate(utils.apply_imagenet_normalization(frames), size=(224, 224))       # trainer.py:280
    assert torch.equal(x, R.preprocess(frames)) and torch.equal(x, R.preprocess_torch(frames))
    for (hi, wi), (ho, wo) in R.RESIZES:
        t = torch.rand(2, 3, hi, wi, generator=torch.Generator().manual_seed(hi * 1000 + wo))
        assert torch.equal(R.preprocess(t, (ho, wo)), R.preprocess_torch(t, (ho, wo))), (hi, wi, ho, wo)
        # normalise-then-resize is resize-then-normalise
        assert torch.equal(R.preprocess(t, (ho, wo)), utils.apply_imagenet_normalization(F.interpolate(t, size=(ho, wo))))

    out, keys = {}, {}
    for name, (layers, bins, gain) in R.NETS.items():
        torch.manual_seed(R.SEED)
        net = trainer.Hopenet(R.Bottleneck, list(layers), bins)
        init_sums = R.state_checksums(net)
        net = R.overwrite(net, head_gain=gain).eval()
        keys[name] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
        with torch.no_grad():
            ang = torch.stack(net(x))
        feat, taps = R.features_of(net, x)
        assert torch.equal(ang, R.angles_of(net, feat))
        mine = R.build(R.RefHopenet, layers, bins, gain)
        assert list(mine.state_dict()) == list(net.state_dict())
        assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), net.state_dict().values()))
        assert torch.equal(mine(x), ang)
        mp = R.max_probs(net, feat)
        fd = [R.rel_l2(feat[i], feat[j]) for i, j in ((0, 1), (0, 2), (1, 2))]
        ad = [(ang[:, i] - ang[:, j]).abs().max().item() for i, j in ((0, 1), (0, 2), (1, 2))]
        ef, ea = R.emulate_bf16(net, x)
        dev = (R.rel_l2(ef, feat), (ea - ang).abs().max().item())
        print(f"{name}: {len(keys[name])} keys, {sum(p.numel() for p in net.parameters())} parameters; max prob "
              f"{mp.min():.3f}..{mp.max():.3f}; feature distances {min(fd):.3f}..{max(fd):.3f}; angle distances "
              f"{min(ad):.3f}..{max(ad):.3f} rad; bf16 emulation: features {dev[0]:.2e} rel-L2, angles {dev[1]:.2e} rad")
        assert 0.05 <= mp.min() and mp.max() <= 0.9, mp
        assert min(fd) >= 0.05, fd
        assert min(ad) >= 1e-2, ad
        out[name] = dict(layers=torch.tensor(layers), num_bins=torch.tensor(bins), head_gain=torch.tensor(gain), seed=torch.tensor(R.SEED),
                         stat_seed=torch.tensor(R.STAT_SEED), input_seed=torch.tensor(R.INPUT_SEED),
                         init_sums=init_sums, state_sums=R.state_checksums(net), input_sum=R.checksum(frames),
                         prep_sum=R.checksum(x), angles=ang, features=feat, taps={str(i): R.sample(t) for i, t in enumerate(taps)},
                         max_prob=mp, bf16_dev=torch.tensor(dev, dtype=torch.float64))
    for path in save_golden(out, "hopenet.pt"):
        print("wrote", path, os.path.getsize(path), "bytes")
    with open(os.path.join(HERE, "hopenet_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote hopenet_keys.json")


if __name__ == "__main__":
    main()
