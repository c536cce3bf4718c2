"""Golden fixtures above 1 MiB are stored in parts, so that no committed file exceeds that size.

A fixture is a (nested) dict of plain tensors.  `save_golden(obj, "name.pt")` writes it whole
when it is small, else as name.part0.pt, name.part1.pt, ...: each part is a list of
[key path, leaf] pairs in the dict's own order, packed up to PART_BYTES.  `load_golden`
reads either form back into the same nested dict (same keys, order, dtypes and values)."""
import glob
import io
import os

import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PART_BYTES = 900 * 1024


def _leaves(obj, path=()):
    if isinstance(obj, dict) and obj:
        for k, v in obj.items():
            yield from _leaves(v, path + (k,))
    else:
        yield list(path), obj


def _size(obj):
    b = io.BytesIO()
    torch.save(obj, b)
    return b.tell()


def _parts(name):
    stem = os.path.join(GOLD, name[:-len(".pt")])
    return sorted(glob.glob(stem + ".part*.pt"), key=lambda p: int(p[len(stem) + len(".part"):-len(".pt")]))


def save_golden(obj, name):
    """-> the files written"""
    for p in _parts(name) + [os.path.join(GOLD, name)]:
        if os.path.exists(p):
            os.remove(p)
    if _size(obj) <= PART_BYTES:
        torch.save(obj, os.path.join(GOLD, name))
        return [os.path.join(GOLD, name)]
    parts, cur, used = [], [], 0
    for path, leaf in _leaves(obj):
        if isinstance(leaf, torch.Tensor):
            leaf = leaf.detach().clone()          # its own storage: a view would drag its base along
        n = _size(leaf)
        if n > PART_BYTES:
            raise ValueError(f"{name}: leaf {path} alone is {n} bytes")
        if cur and used + n > PART_BYTES:
            parts.append(cur)
            cur, used = [], 0
        cur.append([path, leaf])
        used += n
    parts.append(cur)
    files = []
    for i, part in enumerate(parts):
        files.append(os.path.join(GOLD, f"{name[:-len('.pt')]}.part{i}.pt"))
        torch.save(part, files[-1])
    return files


def load_golden(name):
    whole = os.path.join(GOLD, name)
    if os.path.exists(whole):
        return torch.load(whole, weights_only=True)
    files = _parts(name)
    if not files:
        raise FileNotFoundError(whole)
    out = {}
    for f in files:
        for path, leaf in torch.load(f, weights_only=True):
            d = out
            for k in path[:-1]:
                d = d.setdefault(k, {})
            d[path[-1]] = leaf
    return out
